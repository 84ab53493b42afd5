"""Tanks and Temples F-score (precision / recall at a scene's distance threshold tau) of fused point clouds, on the GPU.

Restates the protocol of the public evaluation toolbox for the seven training scenes, which ship a ground-truth scan, a crop
volume and an alignment (DESIGN.md 1.6 holds the rules and where they fix what Open3D leaves open; the agreement with a
toolbox run is unpinned, neither the toolbox nor Open3D was available to compare against):

1. refine the alignment ``trans`` with three rounds of point-to-point ICP with scaling (:func:`register`): crop both clouds, voxel
   down-sample at tau (cap 80 tau), at tau / 2 (cap 20 tau), then every k-th point of clouds above 4 M points (cap 2 tau);
2. transform the prediction, crop both clouds with the scene's polygon volume and voxel down-sample them at tau / 2;
3. capped nearest-neighbour distances prediction -> ground truth and back
   (:func:`cds_mvsnet_amd.pointcloud.nearest_distance`);
4. precision = share of prediction distances below tau, recall = share of ground-truth distances below tau,
   F = 2 P R / (P + R), and the two cumulative curves up to 5 tau.

``python -m cds_mvsnet_amd.tt_eval --datapath <T&T training data> --plydir <outdir> --scenes Barn,Truck`` scores a directory of
fused clouds (``infer --dataset tt --fuse``).  ``<Scene>_trans.txt`` maps the benchmark's own COLMAP reconstruction
(``<Scene>_COLMAP_SfM.log``) onto the scan; a reconstruction made from other cameras, with their own origin, orientation and
scale, is first aligned to that reconstruction from its camera centres, the toolbox's trajectory alignment
(:func:`trajectory_alignment`: a RANSAC over camera-centre correspondences, 100 000 hypotheses of 6, one launch of
cds_ransac_similarity_f64).  ``--cams "<testpath>/{scene}/cams"`` takes the cameras ``infer`` ran with, ``--traj
"<dir>/{scene}.log"`` a trajectory file, ``--export-log DIR`` writes the ``<Scene>.log`` the benchmark website asks for next to
the ``.ply``; the resulting transform replaces ``<Scene>_trans.txt @ init`` as the start of the registration.  The toolbox's
mapping file for video-rate logs is out of scope: both trajectories must list the same cameras in the same order.  The hot
paths are the HIP kernels of ``csrc/registration.hip``, ``csrc/ransac.hip`` and ``csrc/pointcloud.hip``; clouds must be
float32 ROCm tensors (correspondences float64), there is no CPU path.

``--sample_faces [SPACING]`` scores a mesh by its surface: the file is read with ``mesh.read_mesh_ply`` and the samples of its
faces (``mesh.sample_mesh``; SPACING defaults to tau / 2, the voxel of step 2) take the place of its vertices,
which are not added.  Without it a mesh file is scored as the cloud of its vertices, as before.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import re
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, mvs_io
from ._lib import check
from .dtu_eval import _Phases, _mean
from .ops import _stream
from .pointcloud import PointGrid, _grid_args, _points, index_grid, nearest_distance, read_ply_points, voxel_groups

Tensor = torch.Tensor

# distance threshold of the training scenes (the toolbox's scene table)
TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01,
       "Truck": 0.005}
MAX_POINTS = 4_000_000          # round 3 of the registration thins clouds above this to every k-th point
_AXES = {"X": 0, "Y": 1, "Z": 2}


def scene_tau(scene: str, tau: Optional[float] = None) -> float:
    """``tau`` if given, else the table's value; any other scene name needs ``tau``."""
    if tau is not None:
        if not (tau > 0 and math.isfinite(tau)):
            raise ValueError(f"tau must be positive, got {tau}")
        return float(tau)
    if scene not in TAU:
        raise ValueError(f"{scene}: not a Tanks and Temples training scene ({', '.join(TAU)}); pass --tau")
    return TAU[scene]


# ---------------------------------------------------------------------------------------------------------------------
def read_crop(path: str) -> Dict[str, object]:
    """The scene's crop volume ``<Scene>.json`` -> {"orthogonal_axis": "X" | "Y" | "Z", "axis_min", "axis_max",
    "bounding_polygon": float64 [P,3]}."""
    with open(path) as f:
        j = json.load(f)
    for k in ("orthogonal_axis", "axis_min", "axis_max", "bounding_polygon"):
        if k not in j:
            raise ValueError(f"{path}: no {k}")
    axis = str(j["orthogonal_axis"]).upper()
    poly = np.asarray(j["bounding_polygon"], np.float64)
    if axis not in _AXES:
        raise ValueError(f"{path}: orthogonal_axis {j['orthogonal_axis']!r}")
    if poly.ndim != 2 or poly.shape[1] != 3 or not 3 <= poly.shape[0] <= _lib.CROP_MAX_VERTICES:
        raise ValueError(f"{path}: bounding_polygon must hold 3 to {_lib.CROP_MAX_VERTICES} vertices of 3 coordinates")
    return {"orthogonal_axis": axis, "axis_min": float(j["axis_min"]), "axis_max": float(j["axis_max"]),
            "bounding_polygon": poly}


def read_trans(path: str) -> np.ndarray:
    """The 4x4 text matrix of ``<Scene>_trans.txt`` -> float64 [4,4]."""
    m = np.loadtxt(path, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError(f"{path}: expected a 4x4 matrix, got {m.shape}")
    return m


# ---------------------------------------------------------------------------------------------------------------------
def _cloud(t: Tensor, name: str) -> Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a ROCm (cuda) tensor; there is no CPU fallback")
    return _points(t, name)


def _matrix(T, dev) -> Tensor:
    T = np.asarray(T, np.float64)
    if T.shape not in ((4, 4), (3, 4)) or not np.isfinite(T).all():
        raise ValueError(f"transform: expected a finite 4x4 (or 3x4) matrix, got shape {T.shape}")
    return torch.from_numpy(np.ascontiguousarray(T[:3]).reshape(12)).to(dev)


def transform_points(points: Tensor, T) -> Tensor:
    """fp32(T p) for points [N,3]: each row ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3] in float64, every product and sum
    rounded separately, the result rounded once to float32 (cds_transform_points_f32).  ``T``: 4x4 float64 (numpy)."""
    points = _cloud(points, "points")
    out = torch.empty_like(points)
    t = _matrix(T, points.device)
    check(_lib.load().cds_transform_points_f32(points.data_ptr(), points.shape[0], t.data_ptr(), out.data_ptr(), _stream(points)),
          "cds_transform_points_f32")
    return out


def crop_points(points: Tensor, crop: Dict[str, object]) -> Tensor:
    """Keep mask bool [N] of the crop volume of :func:`read_crop` (Open3D's SelectionPolygonVolume), computed in float64:
    ``axis_min <= p[w] <= axis_max`` along the orthogonal axis and, in the other two coordinates (u, v), an odd number of
    polygon edges (a, b) with ``(p[v] < a[v]) != (p[v] < b[v])`` and
    ``a[u] + (p[v] - a[v]) / (b[v] - a[v]) * (b[u] - a[u]) < p[u]`` (cds_polygon_crop_f32)."""
    points = _cloud(points, "points")
    poly = np.ascontiguousarray(np.asarray(crop["bounding_polygon"], np.float64))
    if poly.ndim != 2 or poly.shape[1] != 3 or not 3 <= poly.shape[0] <= _lib.CROP_MAX_VERTICES:
        raise ValueError(f"crop_points: bounding_polygon must hold 3 to {_lib.CROP_MAX_VERTICES} vertices")
    axis = _AXES[str(crop["orthogonal_axis"]).upper()]
    keep = torch.zeros(points.shape[0], dtype=torch.uint8, device=points.device)
    dpoly = torch.from_numpy(poly).to(points.device)
    check(_lib.load().cds_polygon_crop_f32(points.data_ptr(), points.shape[0], dpoly.data_ptr(), poly.shape[0], axis,
                                           float(crop["axis_min"]), float(crop["axis_max"]), keep.data_ptr(), _stream(points)),
          "cds_polygon_crop_f32")
    return keep.bool()


def voxel_down_sample(points: Tensor, voxel: float, return_info: bool = False):
    """Open3D's ``voxel_down_sample``: one point per occupied voxel of side ``voxel``, the mean of the voxel's points.
    Origin ``o = float32(min - voxel / 2)`` per axis, voxel index ``floorf((p - o) / voxel)`` in fp32 (the grid's cell
    expression), mean accumulated in float64 in input order and rounded once (cds_voxel_mean_f32).  The output is ordered
    by ascending voxel key, the grid's key packing: the indices >> 3 of x, y, z (18 bits each), then the low three bits of
    x, y, z.  -> float32 [V,3] (with ``return_info`` also the keys int64 [V] and the counts int64 [V])."""
    points = _cloud(points, "points")
    dev = points.device
    if not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError(f"voxel_down_sample: voxel must be positive, got {voxel}")
    n = points.shape[0]
    if n == 0:
        e = torch.zeros(0, dtype=torch.int64, device=dev)
        return (points.clone(), e, e.clone()) if return_info else points.clone()
    perm, start, ukeys, counts = voxel_groups(points, voxel, "voxel_down_sample")
    out = torch.empty((ukeys.numel(), 3), dtype=torch.float32, device=dev)
    check(_lib.load().cds_voxel_mean_f32(points.data_ptr(), n, perm.data_ptr(), start.data_ptr(), ukeys.numel(), out.data_ptr(),
                                         _stream(points)),
          "cds_voxel_mean_f32")
    return (out, ukeys, counts) if return_info else out


# ---------------------------------------------------------------------------------------------------------------------
class PairSums:
    """The launches of one registration step against a fixed target grid (cds_icp_sums_f64): uploads the 12 doubles of T
    without blocking, runs the two kernels on the current stream and reads the 18 sums back in one copy."""

    def __init__(self, source: Tensor, grid: PointGrid, cap: float, order: Optional[Tensor] = None):
        self.source = _cloud(source, "source")
        if self.source.shape[0] < 1:
            raise ValueError("PairSums: no source points")
        if not grid.indexed:
            raise ValueError("PairSums: the target grid must come from index_grid")
        self.grid, self.cap, self.order = grid, float(cap), order
        dev = self.source.device
        self.t_host = torch.empty(12, dtype=torch.float64).pin_memory()
        self.t_dev = torch.empty(12, dtype=torch.float64, device=dev)
        self.ws = torch.empty(_lib.ICP_MAX_GROUPS * _lib.ICP_SUMS, dtype=torch.float64, device=dev)
        self.out = torch.empty(_lib.ICP_SUMS, dtype=torch.float64, device=dev)

    def launch(self, T: np.ndarray, index: Optional[Tensor] = None, dist: Optional[Tensor] = None) -> Tensor:
        """-> the 18 sums as a device tensor (overwritten by the next launch); nothing is read back."""
        self.t_host.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(T, np.float64)[:3]).reshape(12)))
        self.t_dev.copy_(self.t_host, non_blocking=True)
        s = self.source
        check(_lib.load().cds_icp_sums_f64(s.data_ptr(), self.order.data_ptr() if self.order is not None else None, s.shape[0],
                                           self.t_dev.data_ptr(), *_grid_args(self.grid), self.cap, self.ws.data_ptr(),
                                           self.ws.numel(), self.out.data_ptr(), index.data_ptr() if index is not None else None,
                                           dist.data_ptr() if dist is not None else None, _stream(s)), "cds_icp_sums_f64")
        return self.out

    def __call__(self, T: np.ndarray) -> np.ndarray:
        return self.launch(T).cpu().numpy()                  # the one host read of a step (it also orders the next upload)


def pair_sums(source: Tensor, T, target: Tensor, cap: float, grid: Optional[PointGrid] = None, order: Optional[Tensor] = None,
              return_pairs: bool = False):
    """One registration step on its own: p = fp32(T source), q = the nearest target of p within ``cap``; over the accepted
    pairs the 18 float64 sums [count, sum p (3), sum q (3), sum q p^T (9, row-major), sum |p - q|^2, sum |p|^2] as a device
    tensor (with ``return_pairs`` also dist float32 [M] and index int32 [M])."""
    source = _cloud(source, "source")
    grid = grid if grid is not None else index_grid(_cloud(target, "target"))
    ps = PairSums(source, grid, cap, order)
    if not return_pairs:
        return ps.launch(T).clone()
    index = torch.empty(source.shape[0], dtype=torch.int32, device=source.device)
    dist = torch.empty(source.shape[0], dtype=torch.float32, device=source.device)
    return ps.launch(T, index, dist).clone(), dist, index


def umeyama(sums: np.ndarray, with_scaling: bool = True) -> np.ndarray:
    """The least-squares similarity (rigid without scaling) that maps the p of the pair sums onto their q, float64 4x4:
    covariance ``sum q p^T / n - mean_q mean_p^T`` = U D V^T, R = U E V^T with E = diag(1, 1, +-1) chosen by the sign of
    det(U) det(V) so that R is a rotation, scale = trace(D E) / var_p, t = mean_q - scale R mean_p."""
    s = np.asarray(sums, np.float64)
    n = s[0]
    mp, mq = s[1:4] / n, s[4:7] / n
    cov = s[7:16].reshape(3, 3) / n - np.outer(mq, mp)
    U, D, Vt = np.linalg.svd(cov)
    E = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        E[2] = -1.0
    R = (U * E) @ Vt
    scale = float((D * E).sum() / (s[17] / n - mp @ mp)) if with_scaling else 1.0
    out = np.eye(4)
    out[:3, :3] = scale * R
    out[:3, 3] = mq - scale * (R @ mp)
    return out


def icp(source: Tensor, target: Tensor, cap: float, max_iter: int = 20, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6,
        with_scaling: bool = True, init=None) -> Tuple[np.ndarray, float, float, int]:
    """Point-to-point ICP with Open3D's control flow -> (T float64 4x4, fitness, rmse, iterations).

    Evaluate at T = ``init`` (identity by default): fitness = pairs / M, rmse = sqrt(sum |p - q|^2 / pairs).  Then up to
    ``max_iter`` times: the Umeyama update from the pair sums on the host, T <- update T in float64, re-evaluate with
    p = fp32(T s) from the ORIGINAL source (never from an already rounded cloud), stop once both |d fitness| <
    ``rel_fitness`` and |d rmse| < ``rel_rmse``.  With fewer than 3 pairs T is returned as it stands.  Each evaluation is
    one upload of 12 doubles, the launches of cds_icp_sums_f64 and one host read of the sums."""
    source, target = _cloud(source, "source"), _cloud(target, "target")
    T = np.eye(4) if init is None else np.array(init, np.float64)
    m = source.shape[0]
    if m == 0 or target.shape[0] == 0:
        return T, 0.0, 0.0, 0
    grid = index_grid(target)
    # the lanes follow the cell order of the source at the initial transform: later iterates move it by a fraction of the cap
    order = grid.query_order(transform_points(source, T))
    step = PairSums(source, grid, cap, order)

    def quality(s):
        return s[0] / m, (math.sqrt(s[16] / s[0]) if s[0] > 0 else 0.0)

    s = step(T)
    fit, rmse = quality(s)
    it = 0
    while it < max_iter and s[0] >= 3:
        T = umeyama(s, with_scaling) @ T
        it += 1
        s = step(T)
        nfit, nrmse = quality(s)
        stop = abs(nfit - fit) < rel_fitness and abs(nrmse - rmse) < rel_rmse
        fit, rmse = nfit, nrmse
        if stop:
            break
    return T, float(fit), float(rmse), it


def _every_kth(points: Tensor) -> Tensor:
    n = points.shape[0]
    if n > MAX_POINTS:
        return points[::max(int(round(n / MAX_POINTS)), 1)].contiguous()
    return points


def register(pred: Tensor, gt: Tensor, crop: Dict[str, object], init, tau: float,
             info: Optional[Dict[str, object]] = None) -> np.ndarray:
    """The toolbox's three registration rounds, each starting from the previous transform -> float64 4x4.  Every round crops
    both clouds (the prediction after the transform) and runs :func:`icp` (max_iter 20, with scaling) from the identity,
    composing the result onto the incoming transform: voxel tau with cap 80 tau, voxel tau / 2 with cap 20 tau, then every
    k-th point, k = round(n / 4e6), of a cloud above 4e6 points with cap 2 tau.  ``info`` receives per-round iterations,
    fitness, rmse, point counts and wall milliseconds (whole round, and the ICP alone)."""
    pred, gt = _cloud(pred, "pred"), _cloud(gt, "gt")
    T = np.array(init, np.float64)
    t_crop = gt[crop_points(gt, crop)].contiguous()
    rounds = []
    for voxel, cap in ((tau, 80.0 * tau), (tau / 2.0, 20.0 * tau), (None, 2.0 * tau)):
        t0 = time.time()
        s = transform_points(pred, T)
        s = s[crop_points(s, crop)].contiguous()
        if voxel is None:
            s, t = _every_kth(s), _every_kth(t_crop)
        else:
            s, t = voxel_down_sample(s, voxel), voxel_down_sample(t_crop, voxel)
        t1 = time.time()
        R, fit, rmse, it = icp(s, t, cap)                   # ends with a host read: the wall time covers its device work
        T = R @ T
        rounds.append({"iterations": it, "fitness": fit, "rmse": rmse, "n_source": int(s.shape[0]), "n_target": int(t.shape[0]),
                       "cap": cap, "ms": (time.time() - t0) * 1e3, "icp_ms": (time.time() - t1) * 1e3})
    if info is not None:
        info["rounds"] = rounds
    return T


_register = register            # evaluate() has a flag of that name


def cumulative_curve(d: Tensor, tau: float, bins: int = 500) -> Tensor:
    """Share of the distances below (k + 1) tau / 100 for k = 0 .. bins - 1 (float64 [bins], on the device)."""
    edges = (torch.arange(bins, dtype=torch.float64, device=d.device) + 1.0) * (tau / 100.0)
    s = torch.sort(d.double())[0]
    return torch.searchsorted(s, edges, right=False).double() / max(int(d.numel()), 1)


def evaluate(pred: Tensor, gt: Tensor, crop: Dict[str, object], trans, tau: float, register: bool = True,
             return_arrays: bool = False, timings: Optional[Dict[str, float]] = None) -> Dict[str, object]:
    """Score one predicted cloud pred [N,3] against the ground-truth scan gt [M,3] (float32, device) with the scene's crop
    volume, its alignment ``trans`` (4x4 float64: prediction -> ground-truth frame) and threshold ``tau``.
    -> {"precision", "recall", "fscore", "tau", "transform" (4x4 as lists: ``trans`` refined by :func:`register` unless
    ``register`` is false), "registration" (per-round records), the point counts "n_pred", "n_gt", "n_pred_cropped",
    "n_gt_cropped", "n_pred_sampled", "n_gt_sampled", and the curves "precision_curve" / "recall_curve" (500 bins of
    tau / 100)} (+ the clouds and distances with ``return_arrays``).  An empty side scores 0.  ``timings``: a dict that
    receives the device time of each phase in ms (events on the current stream)."""
    pred, gt = _cloud(pred, "pred"), _cloud(gt, "gt")
    if not (tau > 0 and math.isfinite(tau)):
        raise ValueError(f"evaluate: tau must be positive, got {tau}")
    ev = _Phases(timings)
    reg: Dict[str, object] = {"rounds": []}
    T = np.array(trans, np.float64)
    if register:
        T = _register(pred, gt, crop, T, tau, info=reg)
    ev.mark("registration")
    s = transform_points(pred, T)                    # the ground truth stays in its own frame: the identity changes no bit
    ev.mark("transform")
    s_crop = s[crop_points(s, crop)].contiguous()
    t_crop = gt[crop_points(gt, crop)].contiguous()
    ev.mark("crop")
    s_ds, t_ds = voxel_down_sample(s_crop, tau / 2.0), voxel_down_sample(t_crop, tau / 2.0)
    ev.mark("voxel down-sample")
    cap = 5.0 * tau
    d1 = nearest_distance(s_ds, t_ds, cap)
    ev.mark("pred->gt")
    d2 = nearest_distance(t_ds, s_ds, cap)
    ev.mark("gt->pred")
    n1, n2 = int(d1.numel()), int(d2.numel())
    if n1 == 0 or n2 == 0:
        p = r = f = 0.0
    else:
        p = int((d1.double() < tau).sum()) / n1
        r = int((d2.double() < tau).sum()) / n2
        f = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
    pc, rc = cumulative_curve(d1, tau), cumulative_curve(d2, tau)
    ev.mark("scores")
    ev.finish()
    res: Dict[str, object] = {
        "precision": p, "recall": r, "fscore": f, "tau": float(tau), "transform": T.tolist(), "registration": reg["rounds"],
        "n_pred": int(pred.shape[0]), "n_gt": int(gt.shape[0]), "n_pred_cropped": int(s_crop.shape[0]),
        "n_gt_cropped": int(t_crop.shape[0]), "n_pred_sampled": n1, "n_gt_sampled": n2,
        "precision_curve": pc.cpu().tolist(), "recall_curve": rc.cpu().tolist()}
    if return_arrays:
        res.update({"pred_sampled": s_ds, "gt_sampled": t_ds, "d1": d1, "d2": d2})
    return res


# ---------------------------------------------------------------------------------------------------------------------
def read_log_trajectory(path: str) -> np.ndarray:
    """The toolbox's ``.log`` trajectory -> camera-to-world poses float64 [M,4,4].  Per camera one metadata line of three
    integers, then the four rows of the matrix; blank lines between cameras are skipped."""
    with open(path) as f:
        lines = [(no, ln.split()) for no, ln in enumerate(f, 1) if ln.strip()]
    poses = []
    for i in range(0, len(lines), 5):
        no, meta = lines[i]
        try:
            if len(meta) != 3:
                raise ValueError
            [int(v) for v in meta]
        except ValueError:
            raise ValueError(f"{path}:{no}: expected a metadata line of three integers, got {' '.join(meta)!r}") from None
        rows = lines[i + 1:i + 5]
        if len(rows) < 4:
            raise ValueError(f"{path}:{no}: camera {len(poses)} has {len(rows)} matrix rows, expected 4")
        m = np.empty((4, 4), np.float64)
        for r, (rno, fields) in enumerate(rows):
            try:
                if len(fields) != 4:
                    raise ValueError
                m[r] = [float(v) for v in fields]
            except ValueError:
                raise ValueError(f"{path}:{rno}: expected a matrix row of four numbers, got {' '.join(fields)!r}") from None
        poses.append(m)
    return np.stack(poses) if poses else np.zeros((0, 4, 4), np.float64)


def write_log_trajectory(path: str, poses) -> None:
    """The inverse of :func:`read_log_trajectory`: camera i as the metadata line ``i i 0`` and four rows, every number
    written so that it reads back to the same float64."""
    poses = np.asarray(poses, np.float64)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        raise ValueError(f"write_log_trajectory: expected poses [M,4,4], got {poses.shape}")
    with open(path, "w") as f:
        for i, m in enumerate(poses):
            f.write(f"{i} {i} 0\n")
            for row in m:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")


def camera_poses_from_cams(folder: str) -> np.ndarray:
    """Camera-to-world poses float64 [M,4,4] of an MVSNet ``cams`` folder: ``%08d_cam.txt`` in ascending id, the
    world-to-camera extrinsic of :func:`mvs_io.read_saved_cam` inverted in float64."""
    if not os.path.isdir(folder):
        raise FileNotFoundError(f"{folder} not found")
    names = sorted(n for n in os.listdir(folder) if re.fullmatch(r"\d{8}_cam\.txt", n))
    if not names:
        raise FileNotFoundError(f"{folder}: no %08d_cam.txt files")
    return np.stack([np.linalg.inv(mvs_io.read_saved_cam(os.path.join(folder, n))[0].astype(np.float64)) for n in names])


def _correspondences(t: Tensor, name: str) -> Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a ROCm (cuda) tensor; there is no CPU fallback")
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name}: expected a float64 tensor [N,3], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def ransac_similarity(src: Tensor, dst: Tensor, threshold: float, k: int = 6, iterations: int = 100_000, seed: int = 0,
                      return_all: bool = False):
    """RANSAC for the similarity that maps src onto dst (float64 [N,3] device tensors, correspondence i <-> i), one launch
    of cds_ransac_similarity_f64 and one host read: ``iterations`` hypotheses of ``k`` distinct correspondences drawn from
    (seed, hypothesis) alone, Umeyama with scaling on each, scored over all N with ``|T src_i - dst_i| < threshold``; the
    winner has the most inliers, then the smallest sum of squared inlier distances, then the smallest index; no refit.
    -> (T float64 4x4, {"index", "count", "fitness" = count / N, "rmse" = sqrt(err2 / count)}); with no accepted hypothesis
    index -1, count 0 and the identity.  ``return_all`` adds (count int32 [iterations], err2 float64 [iterations]) of every
    hypothesis as device tensors (a rejected one: 0, +inf)."""
    src, dst = _correspondences(src, "src"), _correspondences(dst, "dst")
    if src.shape != dst.shape or src.device != dst.device:
        raise ValueError(f"ransac_similarity: src {tuple(src.shape)} and dst {tuple(dst.shape)} must match, on one device")
    if not _lib.RANSAC_MIN_SAMPLE <= k <= _lib.RANSAC_MAX_SAMPLE:
        raise ValueError(f"ransac_similarity: k must be {_lib.RANSAC_MIN_SAMPLE}..{_lib.RANSAC_MAX_SAMPLE}, got {k}")
    if not (threshold >= 0 and math.isfinite(threshold)) or iterations < 0 or not 0 <= seed < 2 ** 64:
        raise ValueError(f"ransac_similarity: threshold {threshold}, iterations {iterations}, seed {seed}")
    dev, n, H = src.device, src.shape[0], int(iterations)
    ws = torch.empty(max((H + 255) // 256, 1) * _lib.RANSAC_RECORD, dtype=torch.float64, device=dev)
    out = torch.empty(_lib.RANSAC_RECORD, dtype=torch.float64, device=dev)
    count = torch.empty(H, dtype=torch.int32, device=dev) if return_all else None
    err2 = torch.empty(H, dtype=torch.float64, device=dev) if return_all else None
    check(_lib.load().cds_ransac_similarity_f64(src.data_ptr(), dst.data_ptr(), n, H, int(k), float(threshold), int(seed),
                                                ws.data_ptr(), ws.numel(), out.data_ptr(),
                                                count.data_ptr() if return_all else None,
                                                err2.data_ptr() if return_all else None, _stream(src)),
          "cds_ransac_similarity_f64")
    rec = out.cpu().numpy()
    T = np.eye(4)
    T[:3] = rec[3:].reshape(3, 4)
    c = int(rec[1])
    info = {"index": int(rec[0]), "count": c, "fitness": c / n if n else 0.0, "rmse": math.sqrt(rec[2] / c) if c else 0.0}
    return (T, info, count, err2) if return_all else (T, info)


def trajectory_alignment(est_poses, ref_poses, trans, threshold: float = 0.2, k: int = 6, iterations: int = 100_000,
                         seed: int = 0, device="cuda", info: Optional[Dict[str, object]] = None) -> np.ndarray:
    """The toolbox's ``trajectory_alignment`` with its constants -> float64 4x4 from the estimate's frame to the
    ground-truth frame.  Source: the camera centres of ``est_poses`` (camera-to-world [M,4,4]); target: ``trans`` (the
    scene's ``_trans.txt``) applied to the centres of ``ref_poses`` (the scene's ``_COLMAP_SfM.log``), camera i <-> camera
    i; :func:`ransac_similarity` between them.  Both must hold the same cameras (the toolbox's mapping file for video-rate
    logs is out of scope): unequal counts raise, as does a result with no inlier or fewer than ``k``.  ``info`` receives
    index, count, fitness, rmse and the transform."""
    est, ref = np.asarray(est_poses, np.float64), np.asarray(ref_poses, np.float64)
    for name, a in (("est_poses", est), ("ref_poses", ref)):
        if a.ndim != 3 or a.shape[1:] != (4, 4):
            raise ValueError(f"trajectory_alignment: {name} must be [M,4,4], got {a.shape}")
    if len(est) != len(ref):
        raise ValueError(f"trajectory_alignment: {len(est)} estimated cameras against {len(ref)} reference cameras; "
                         "both trajectories must list the same cameras")
    trans = np.asarray(trans, np.float64)
    if trans.shape != (4, 4):
        raise ValueError(f"trajectory_alignment: trans must be 4x4, got {trans.shape}")
    src = np.ascontiguousarray(est[:, :3, 3])
    dst = np.ascontiguousarray(ref[:, :3, 3] @ trans[:3, :3].T + trans[:3, 3])
    T, r = ransac_similarity(torch.from_numpy(src).to(device), torch.from_numpy(dst).to(device), threshold, k, iterations, seed)
    if r["count"] == 0 or r["count"] < k:
        raise ValueError(f"trajectory_alignment: no similarity fits the {len(est)} camera centres within {threshold} "
                         f"({r['count']} inliers, {k} needed)")
    if info is not None:
        info.update(r, transform=T.tolist())
    return T


# ---------------------------------------------------------------------------------------------------------------------
def scene_names(testlist: Optional[str], scenes: Optional[str]) -> List[str]:
    if testlist:
        return mvs_io.read_testlist(testlist)
    return [s.strip() for s in scenes.split(",") if s.strip()]


def scene_paths(datapath: str, scene: str) -> Dict[str, str]:
    d = os.path.join(datapath, scene)
    return {"ply": os.path.join(d, f"{scene}.ply"), "crop": os.path.join(d, f"{scene}.json"),
            "trans": os.path.join(d, f"{scene}_trans.txt")}


def main(argv: Optional[Sequence[str]] = None) -> Dict[str, object]:
    ap = argparse.ArgumentParser(prog="python -m cds_mvsnet_amd.tt_eval",
                                 description="Tanks and Temples precision / recall / F-score of fused point clouds, on the GPU")
    ap.add_argument("--datapath", required=True, help="the T&T training data: <Scene>/<Scene>.ply, <Scene>.json, <Scene>_trans.txt "
                                                     "(with --traj / --cams also <Scene>_COLMAP_SfM.log)")
    ap.add_argument("--plydir", required=True, help="folder of the fused clouds (infer --dataset tt --fuse --outdir)")
    grp = ap.add_mutually_exclusive_group(required=True)
    grp.add_argument("--testlist", help="file with one scene per line")
    grp.add_argument("--scenes", help="comma-separated scene names, e.g. Barn,Truck")
    ap.add_argument("--ply", default="{scene}.ply", help="file name of a scene's cloud; {scene} = Barn")
    ap.add_argument("--tau", type=float, help="distance threshold; required for a scene outside the training set")
    start = ap.add_mutually_exclusive_group()
    start.add_argument("--init", help="4x4 text matrix right-multiplied onto <Scene>_trans.txt")
    start.add_argument("--traj", help="the reconstruction's camera trajectory (.log, camera-to-world); {scene} = Barn.  Aligned to "
                                      "<Scene>_COLMAP_SfM.log from the camera centres; the result replaces <Scene>_trans.txt")
    start.add_argument("--cams", help="the same from the cameras infer ran with: the folder of %%08d_cam.txt, e.g. "
                                      "\"<testpath>/{scene}/cams\"")
    ap.add_argument("--export-log", metavar="DIR", help="with --cams: write <Scene>.log, the trajectory file the benchmark asks for")
    ap.add_argument("--seed", type=int, default=0, help="seed of the trajectory alignment's RANSAC")
    ap.add_argument("--no-register", action="store_true", help="score at the initial transform, without the ICP rounds")
    ap.add_argument("--json", help="write the per-scene and mean results here")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--sample_faces", nargs="?", type=float, const=0.0, default=None, metavar="SPACING",
                    help="the files are meshes: score the samples of their faces (sub-triangle centroids, edges of at most "
                         "SPACING, default tau / 2, the voxel the toolbox samples at) instead of their vertices")
    args = ap.parse_args(argv)
    if args.sample_faces is not None and not (args.sample_faces >= 0 and math.isfinite(args.sample_faces)):
        ap.error(f"--sample_faces must be positive, got {args.sample_faces}")

    dev = torch.device(args.device)
    if dev.type != "cuda":
        raise SystemExit("tt_eval runs on the GPU only (--device cuda[:N])")
    if args.export_log and not args.cams:
        ap.error("--export-log needs --cams")
    init = read_trans(args.init) if args.init else np.eye(4)
    aligned = bool(args.traj or args.cams)
    jobs = []
    for scene in scene_names(args.testlist, args.scenes):        # resolve every file and tau before the first scene is scored
        try:
            tau = scene_tau(scene, args.tau)
        except ValueError as e:
            ap.error(str(e))
        ply = os.path.join(args.plydir, args.ply.format(scene=scene))
        paths = scene_paths(args.datapath, scene)
        if aligned:
            paths["sfm_log"] = os.path.join(args.datapath, scene, f"{scene}_COLMAP_SfM.log")
        if args.traj:
            paths["traj"] = args.traj.format(scene=scene)
        for p in [ply] + list(paths.values()):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"{scene}: {p} not found")
        if args.cams:
            paths["cams"] = args.cams.format(scene=scene)
            if not os.path.isdir(paths["cams"]):
                raise FileNotFoundError(f"{scene}: {paths['cams']} not found")
        jobs.append((scene, tau, ply, paths))
    if args.export_log:
        os.makedirs(args.export_log, exist_ok=True)
    per_scene: Dict[str, Dict[str, object]] = {}
    with torch.cuda.device(dev):
        for scene, tau, ply, paths in jobs:
            t0 = time.time()
            gt = torch.from_numpy(read_ply_points(paths["ply"])).to(dev)
            sampled = None
            if args.sample_faces is None:
                pred = torch.from_numpy(read_ply_points(ply)).to(dev)
            else:
                from .mesh import sample_file
                spacing = args.sample_faces if args.sample_faces != 0.0 else tau / 2.0
                try:
                    out, sampled = sample_file(ply, spacing, dev)
                except ValueError as e:                          # a cloud, or a spacing too fine for the mesh
                    raise SystemExit(f"{scene}: --sample_faces: {e}") from None
                pred = out["points"]
            start, traj = read_trans(paths["trans"]) @ init, None
            if aligned:
                est = camera_poses_from_cams(paths["cams"]) if args.cams else read_log_trajectory(paths["traj"])
                if args.export_log:
                    write_log_trajectory(os.path.join(args.export_log, f"{scene}.log"), est)
                traj = {}
                start = trajectory_alignment(est, read_log_trajectory(paths["sfm_log"]), read_trans(paths["trans"]),
                                             seed=args.seed, device=dev, info=traj)
            r = evaluate(pred, gt, read_crop(paths["crop"]), start, tau, register=not args.no_register)
            if traj is not None:
                r["trajectory"] = traj
            if sampled is not None:
                r.update(n_faces=sampled["faces"], n_sampled=sampled["points"], sample_spacing=spacing)
            per_scene[scene] = r
            print(f"{scene}: precision {r['precision']:.4f}  recall {r['recall']:.4f}  f-score {r['fscore']:.4f}  "
                  f"(tau {tau:g}, {r['n_pred_sampled']} / {r['n_gt_sampled']} points, {time.time() - t0:.1f} s)"
                  + (f"  [{r['n_sampled']} samples of {r['n_faces']} faces]" if sampled is not None else ""), flush=True)
    mean = {k: _mean([r[k] for r in per_scene.values()]) for k in ("precision", "recall", "fscore")}
    print(f"mean over {len(per_scene)} scenes: precision {mean['precision']:.4f}  recall {mean['recall']:.4f}  "
          f"f-score {mean['fscore']:.4f}")
    out = {"scenes": per_scene, "mean": mean, "settings": {"tau": args.tau, "register": not args.no_register}}
    if aligned:                                                      # without the alignment the output stays as it was
        out["settings"]["seed"] = args.seed
    if args.sample_faces is not None:                                # likewise; 0: tau / 2 of each scene
        out["settings"]["sample_faces"] = args.sample_faces if args.sample_faces != 0.0 else "tau / 2"
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
