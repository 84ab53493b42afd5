"""Gipuma-style depth-map fusion on the GPU: the reference's ``--filter_method gipuma`` (gipuma.py) without fusibile.

The reference filters the depth maps by probability (gipuma.py:153-175), converts them to gipuma's file layout
(gipuma.py:20-150) and runs fusibile, an external CUDA program (gipuma.py:178-195).  This module runs the fusion itself,
with the kernels of ``csrc/gipuma.hip``, and can still write fusibile's inputs (:func:`export_fusibile_inputs`).

The rule (it follows fusibile's fusion, Galliani et al., ICCV 2015, and fixes the points marked (def) where fusibile's
behaviour is not known or not consistent with itself).  Inputs per scan, from the ``infer`` output folder ``<out>/<scan>/``:
the views are the ids of ``images/%08d.jpg`` in ascending order, and every view is checked against every other view;
per view v the depth D_v, the three-stage confidence C_v, the camera K_v, E_v and the RGB image I_v (uint8).  All views have
one h x w.  Parameters and defaults are the reference's: prob_threshold (p1, p2, p3) = 0, 0, 0, disp_threshold = 0.2,
num_consistent = 3, depth_min = 0.001, depth_max = 100000; there is no normal-angle test (the reference disables it).

1. D'_v(p) = D_v(p) if C_v[0](p) > p1 and C_v[1](p) > p2 and C_v[2](p) > p3, otherwise 0.
2. Per view, on the host in float64 and then cast to float32: P_v = K_v E_v[:3, :] (what the reference writes as ``.P``),
   Minv_v = inverse(P_v[:, :3]), p4_v = P_v[:, 3], centre c_v = -Minv_v p4_v; per ordered pair
   fb_rj = K_r[0, 0] |c_r - c_j| (def: f is read from K, not from decomposing P).
3. used_v starts at 0.  The reference views r are visited in ascending order, one after another.  For every pixel
   p = (x, y) of r (integer coordinates, no +0.5) with d = D'_r(p): skip p if used_r(p) is set or d is not in
   (depth_min, depth_max); X = Minv_r (d x - p4_r.x, d y - p4_r.y, d - p4_r.z), S = X, rgb = I_r(p), n = 0; for each j != r
   ascending: (a, b, z) = P_j (X, 1); skip j if z <= 0 (def); u = a / z, v = b / z; skip unless 0 <= u < w and 0 <= v < h;
   iu = min(floor(u + 0.5), w - 1), iv = min(floor(v + 0.5), h - 1); dj = D'_j(iu, iv); skip if dj is not in
   (depth_min, depth_max) (def); skip unless |fb_rj / z - fb_rj / dj| < disp_threshold; otherwise n += 1,
   S += Minv_j (dj iu - p4_j.x, dj iv - p4_j.y, dj - p4_j.z), rgb += I_j(iu, iv) and (j, iu, iv) is remembered (def: the
   depth sample, the 3D point and the used mark all use the same rounded pixel).  If n >= num_consistent the point
   S / (n + 1) is emitted with colour rgb // (n + 1) and used_j(iu, iv) = 1 for every remembered (j, iu, iv).  A pixel
   already used in j still counts as evidence for a later r; it only never starts a point.
4. The points are written in the order r, y, x with :func:`fusion.write_ply` to ``<out>/<scan>.ply``.

The fp32 arithmetic is part of the definition: its operation order is in the header comment of ``csrc/gipuma.hip``.

    python -m cds_mvsnet_amd.gipuma --outdir <out> --testlist <list> [--prob_threshold 0,0,0] [--disp_threshold 0.2]
        [--num_consistent 3] [--export_fusibile]

re-fuses saved depth maps without running the network again.
"""
from __future__ import annotations

import argparse
import os
import shutil
import struct
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .mvs_io import ScanFolder, read_testlist, write_pfm
from .ply import write_ply

DEPTH_MIN = 0.001
DEPTH_MAX = 100000.0
GIPUMA_PREFIX = "2333__"     # the reference's name prefix of the per-view depth folders (gipuma.py:135)


def _thresholds(prob_threshold) -> Tuple[float, float, float]:
    if isinstance(prob_threshold, str):
        prob_threshold = prob_threshold.split(",")
    th = tuple(float(p) for p in prob_threshold)
    if len(th) != 3:
        raise ValueError(f"three probability thresholds expected, got {prob_threshold!r}")
    return th


def projection_matrix(cam: np.ndarray) -> np.ndarray:
    """cam [2,4,4] (extrinsic; intrinsic in [1,:3,:3]) -> P [3,4] float64 = K E[:3], computed as the reference's
    ``mvsnet_to_gipuma_cam`` computes it (a 4x4 float64 intrinsic with the float32 extrinsic)."""
    k4 = np.zeros((4, 4))
    k4[:3, :3] = np.asarray(cam[1, :3, :3], np.float32)
    return np.matmul(k4, np.asarray(cam[0], np.float32))[:3]


def camera_constants(cams: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """cams [V,2,4,4] -> (views [V,24] float32: P row-major (12), Minv (9), 3 zeros; fb [V,V] float32) (step 2)."""
    cams = np.asarray(cams, np.float32)
    V = cams.shape[0]
    views = np.zeros((V, 24), np.float32)
    centres = np.zeros((V, 3))
    for v in range(V):
        P = projection_matrix(cams[v])
        minv = np.linalg.inv(P[:, :3])
        centres[v] = -minv @ P[:, 3]
        views[v, :12] = P.reshape(-1)
        views[v, 12:21] = minv.reshape(-1)
    f = cams[:, 1, 0, 0].astype(np.float64)
    fb = f[:, None] * np.linalg.norm(centres[:, None, :] - centres[None, :, :], axis=-1)
    return views, fb.astype(np.float32)


def fuse_views(depths: torch.Tensor, confs: torch.Tensor, cams, images: torch.Tensor,
               prob_threshold: Sequence[float] = (0.0, 0.0, 0.0), disp_threshold: float = 0.2, num_consistent: int = 3,
               depth_min: float = DEPTH_MIN, depth_max: float = DEPTH_MAX) -> Dict[str, torch.Tensor]:
    """The rule on device tensors: depths [V,h,w], confs [V,3,h,w] (float32), images [V,h,w,3] (uint8); cams [V,2,4,4]
    (any device: the constants are computed on the host).  -> {"points" [N,3] float32, "colors" [N,3] uint8, "ref_view" [N]
    int32, "used" [V,h,w] bool}, all on the device, the points in the order (r, y, x).  The reference views run one after
    another on the current stream; the host reads back one number (the point count)."""
    for name, t in (("depths", depths), ("confs", confs), ("images", images)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"fuse_views: {name} must be a ROCm (cuda) tensor; there is no CPU fallback")
    if depths.dim() != 3:
        raise ValueError(f"fuse_views: depths must be [V,h,w], got {tuple(depths.shape)}")
    V, h, w = depths.shape
    cams = cams.detach().cpu().numpy() if isinstance(cams, torch.Tensor) else np.asarray(cams)
    if tuple(confs.shape) != (V, 3, h, w) or tuple(images.shape) != (V, h, w, 3) or tuple(cams.shape) != (V, 2, 4, 4):
        raise ValueError(f"fuse_views: confs {tuple(confs.shape)}, images {tuple(images.shape)} and cams {tuple(cams.shape)} "
                         f"do not match depths {tuple(depths.shape)}")
    dev = depths.device
    views, fb = camera_constants(cams)
    views_d, fb_d = torch.from_numpy(views).to(dev), torch.from_numpy(fb).to(dev)
    with torch.cuda.device(dev):
        filt, rgb = ops.gipuma_prob_filter(depths.float().contiguous(), confs.float().contiguous(), images.contiguous(),
                                           _thresholds(prob_threshold))
        tiles = ops.gipuma_tiles(V * h * w)
        used = torch.zeros((V, h, w), dtype=torch.uint8, device=dev)
        emit = torch.zeros(tiles * 4096, dtype=torch.uint8, device=dev)
        records = torch.empty((V, h, w, 4), dtype=torch.int32, device=dev)
        for r in range(V):
            ops.gipuma_fuse_view(r, filt, rgb, views_d, fb_d, depth_min, depth_max, disp_threshold, num_consistent, used, emit,
                                 records)
        tile_off, total = ops.gipuma_scan(emit)
        n = int(total.item())
        points, colors, ref = ops.gipuma_compact(emit, records, tile_off, n)
    return {"points": points, "colors": colors.view(torch.uint8).view(n, 4)[:, :3], "ref_view": ref, "used": used.bool()}


# ------------------------------------------------------------------------------------------------------------- files
def load_scan(scan_folder: str) -> Dict[str, np.ndarray]:
    """depths [V,h,w], confs [V,3,h,w] float32, cams [V,2,4,4], images [V,h,w,3] uint8 and ids [V] of one ``infer`` scan
    folder, the views in ascending id (the views fusibile is given); ValueError if the views differ in size."""
    scan = ScanFolder(scan_folder)
    return scan.load_views(scan.view_ids())


def filter_scan(scan_folder: str, plyfilename: str, prob_threshold: Sequence[float] = (0.0, 0.0, 0.0),
                disp_threshold: float = 0.2, num_consistent: int = 3, depth_min: float = DEPTH_MIN,
                depth_max: float = DEPTH_MAX, device: str = "cuda", merge_voxel: Optional[float] = None,
                merge_min_points: int = 1, outlier_nb: int = 0, outlier_std: float = 2.0, outlier_radius: float = 0.0,
                outlier_min_nb: int = 0, outlier_max_dist: Optional[float] = None) -> Dict[str, int]:
    """Fuse one ``infer`` scan folder into a PLY at ``plyfilename`` (steps 1-4). -> {"points", "views"}.  ``merge_voxel``: the
    emitted cloud is merged to one point per occupied voxel of that side, voxels with fewer than ``merge_min_points`` points
    dropped (:func:`pointcloud.merge_voxels`); the dict then also has "merged_from".  ``outlier_*``: the cloud,
    merged or not, goes through :func:`pointcloud.remove_outliers` as in :func:`fusion.filter_depth`."""
    from .pointcloud import check_outlier_args
    check_outlier_args(outlier_nb, outlier_std, outlier_radius, outlier_min_nb, outlier_max_dist)
    s = load_scan(scan_folder)
    out = fuse_views(torch.from_numpy(s["depths"]).to(device), torch.from_numpy(s["confs"]).to(device), s["cams"],
                     torch.from_numpy(s["images"]).to(device), prob_threshold, disp_threshold, num_consistent, depth_min,
                     depth_max)
    info = {"points": int(out["points"].shape[0]), "views": int(len(s["ids"]))}
    if merge_voxel is not None:
        from .pointcloud import merge_voxels
        out = merge_voxels(out["points"], out["colors"], float(merge_voxel), min_points=merge_min_points)
        info = {"points": int(out["points"].shape[0]), "views": info["views"], "merged_from": info["points"]}
    if outlier_nb > 0 or outlier_radius > 0:
        from .fusion import clean_cloud
        pts, col, _ = clean_cloud(out["points"], out["colors"], None,
                                  dict(nb_neighbors=outlier_nb, std_ratio=outlier_std, radius=outlier_radius,
                                       min_neighbors=outlier_min_nb, max_dist=outlier_max_dist), info)
        out = {"points": pts, "colors": col}
    write_ply(plyfilename, out["points"].cpu().numpy(), out["colors"].cpu().numpy())
    return info


def write_dmb(path: str, image: np.ndarray) -> None:
    """gipuma's ``.dmb``: int32 type 1, height, width, channels, then the float32 payload channel by channel, row-major."""
    image = np.asarray(image, np.float32)
    h, w = image.shape[:2]
    c = image.shape[2] if image.ndim == 3 else 1
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", 1, h, w, c))
        f.write(np.ascontiguousarray(image.reshape(h, w, c).transpose(2, 0, 1)).astype("<f4").tobytes())


def read_dmb(path: str) -> np.ndarray:
    """A ``.dmb`` file -> float32 [h,w] or [h,w,c] (single-size axes squeezed, as the reference's reader does)."""
    with open(path, "rb") as f:
        _, h, w, c = struct.unpack("<4i", f.read(16))
        data = np.frombuffer(f.read(), dtype="<f4")
    if data.size != h * w * c:
        raise ValueError(f"{path}: payload of {data.size} floats, header says {h}x{w}x{c}")
    return data.astype(np.float32).reshape(c, h, w).transpose(1, 2, 0).squeeze()


def write_projection(path: str, P: np.ndarray) -> None:
    """gipuma's ``.P`` camera: three rows of four numbers (``str`` of the float64 values), each followed by a space."""
    with open(path, "w") as f:
        for row in P:
            f.write("".join(str(x) + " " for x in row) + "\n")
        f.write("\n")


def export_fusibile_inputs(scan_folder: str, prob_threshold: Sequence[float] = (0.0, 0.0, 0.0)) -> str:
    """Write what the reference's ``probability_filter`` and ``mvsnet_to_gipuma`` write (gipuma.py:106-175):
    ``depth_est/<id>_prob_filtered.pfm`` and ``points_mvsnet/`` with ``cams/<image>.P``, ``images/``,
    ``2333__<id>/disp.dmb`` and ``normals.dmb`` (1/sqrt(3) where the depth is positive).  -> the points_mvsnet folder."""
    th = _thresholds(prob_threshold)
    scan = ScanFolder(scan_folder)
    point_folder = os.path.join(scan_folder, "points_mvsnet")
    for sub in ("cams", "images"):
        os.makedirs(os.path.join(point_folder, sub), exist_ok=True)
    for vid in scan.view_ids():
        stem, name = f"{vid:08d}", f"{vid:08d}.jpg"
        depth = scan.depth(vid)
        depth[~(scan.conf(vid) > np.array(th, np.float32).reshape(3, 1, 1)).all(0)] = 0
        write_pfm(scan.path("depth_est", vid, "_prob_filtered.pfm"), depth)
        write_projection(os.path.join(point_folder, "cams", name + ".P"), projection_matrix(scan.cam(vid)))
        shutil.copyfile(os.path.join(scan_folder, "images", name), os.path.join(point_folder, "images", name))
        view_dir = os.path.join(point_folder, GIPUMA_PREFIX + stem)
        os.makedirs(view_dir, exist_ok=True)
        write_dmb(os.path.join(view_dir, "disp.dmb"), depth)
        normal = np.where(depth > 0, np.float32(1.0 / 1.732050808), np.float32(0.0)).astype(np.float32)
        write_dmb(os.path.join(view_dir, "normals.dmb"), np.repeat(normal[:, :, None], 3, axis=2))
    return point_folder


# --------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--outdir", required=True, help="the infer output folder: <outdir>/<scan>/{depth_est,confidence,cams,images}")
    ap.add_argument("--testlist", required=True, help="text file with one scan name per line")
    ap.add_argument("--prob_threshold", default="0.0,0.0,0.0", help="per-stage confidence thresholds (test.py:68)")
    ap.add_argument("--disp_threshold", type=float, default=0.2)
    ap.add_argument("--num_consistent", type=int, default=3)
    ap.add_argument("--export_fusibile", action="store_true",
                    help="also write fusibile's inputs (depth_est/*_prob_filtered.pfm, points_mvsnet/)")
    from .fusion import add_cloud_args, add_outlier_args, outlier_kwargs
    add_cloud_args(ap, normals=False)          # normals are not implemented for this method
    add_outlier_args(ap)
    args = ap.parse_args(argv)
    args.outliers = outlier_kwargs(args, ap)
    args.prob_threshold = _thresholds(args.prob_threshold)
    return args


def main(argv=None) -> Dict[str, Dict[str, int]]:
    args = parse_args(argv)
    scans = read_testlist(args.testlist)
    out = {}
    for scan in scans:
        folder = os.path.join(args.outdir, scan)
        if args.export_fusibile:
            export_fusibile_inputs(folder, args.prob_threshold)
        out[scan] = filter_scan(folder, os.path.join(args.outdir, f"{scan}.ply"), args.prob_threshold, args.disp_threshold,
                                args.num_consistent, merge_voxel=args.merge_voxel, merge_min_points=args.merge_min_points,
                                **args.outliers)
        merged = f", merged from {out[scan]['merged_from']}" if "merged_from" in out[scan] else ""
        from .fusion import format_outliers
        print(f"{scan}.ply: {out[scan]['points']} points from {out[scan]['views']} views{merged}{format_outliers(out[scan])}",
              flush=True)
    return out


if __name__ == "__main__":
    main()
