"""Depth-map filtering and point-cloud fusion on the GPU.

Mirrors step 2 of the reference's ``test.py`` (``filter_depth``, test.py:324-383, built on fusion.py): for every
reference view read back ``depth_est/ confidence/ cams/ images/`` written by :mod:`cds_mvsnet_amd.infer`, keep the
pixels whose three stage confidences exceed ``conf`` and that re-project consistently (pixel distance < ``thres_disp``,
relative depth difference < 1 %) into at least ``thres_view`` source views, average the consistent depths and emit the
world-space points with their colours as one binary PLY.

All per-pixel work is one launch of ``cds_depth_fusion_f32`` per reference view; the host side only reads files, inverts
the 3x3 / 4x4 camera matrices (fp32, CPU) and compacts the masked points.

``method="dynamic"`` replaces the fixed threshold pair by the dynamic consistency check of DESIGN §1.7
(``cds_depth_fusion_dynamic_f32``, rule in include/cds_mvsnet_hip.h): a view agrees at level n when it re-projects within
n * ``dist_base`` pixels and n * ``rel_base`` relative depth, and a pixel is kept when, for some n in ``n_views``, at least n
views agree at level n.  Same inputs, same files, same PLY.  The rule is this project's own statement of the check that
D2HC-RMVSNet popularised; no outside implementation was available to compare against.

    python -m cds_mvsnet_amd.fusion --testpath <scenes> --outdir <out> --testlist <list> [--filter_method normal|dynamic]
        [--conf 0,0,0] [--thres_disp 1.0] [--thres_view 3] [--dyn_dist_base 0.25] [--dyn_rel_base 0.000769] [--dyn_views 2,10]

        [--normals [--normal_radius 2] [--normal_jump 0.01] [--normal_min_pts 6]] [--merge_voxel SIZE [--merge_min_points K]]

re-fuses saved depth maps (``<out>/<scan>/``, pairs from ``<scenes>/<scan>/pair.txt``) into ``<out>/<scan>.ply`` without
running the network again.

``--normals`` and ``--merge_voxel`` make the cloud usable outside this project: every point gets the oriented
normal of its reference view's depth map (``cds_depth_normals_f32``; it faces that camera), and the concatenation of the views,
in which a surface seen by ten views is written ten times, is merged to one point per occupied voxel (``cds_voxel_merge_f32``).
Whatever the options, the views' points stay on the device until the scan is done and are downloaded once.

``--outlier_nb K [--outlier_std 2.0]`` and ``--outlier_radius r --outlier_min_nb n`` (``--outlier_max_dist d``) remove the cloud's
outliers on the device before it is written, after the merge when both are given (:func:`pointcloud.remove_outliers`,
DESIGN §1.16); ``--from_ply "<out>/{scan}.ply"`` does that to saved clouds, without the fusion and without ``--testpath``.

``filter_depth(collect=...)`` hands the same pass to a later stage: per reference view the fused depth, the mask, the image, the
camera and the kept points, on the device.  :mod:`cds_mvsnet_amd.mesh` builds a triangle mesh from them.
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .mvs_io import ScanFolder, read_pair_file, read_saved_cam as read_fusion_cam, read_testlist   # noqa: F401
from .ply import read_ply, read_ply_full, write_ply                                                # noqa: F401


def camera_chains(ref_cam: torch.Tensor, src_cams: torch.Tensor) -> torch.Tensor:
    """ref_cam [2,4,4], src_cams [V,2,4,4] (CPU fp32) -> [V,100] blocks for cds_depth_fusion_f32:
    Kinv_ref Einv_ref E_src K_src | Kinv_src Einv_src E_ref K_ref (fusion.py:24-46 applies them in this order)."""
    ref_cam = ref_cam.detach().to("cpu", torch.float32)
    src_cams = src_cams.detach().to("cpu", torch.float32)
    k_ref, e_ref = ref_cam[1, :3, :3], ref_cam[0]
    kinv_ref, einv_ref = torch.inverse(k_ref), torch.inverse(e_ref)
    rows = []
    for cam in src_cams:
        k_src, e_src = cam[1, :3, :3], cam[0]
        rows.append(torch.cat([kinv_ref.reshape(9), einv_ref.reshape(16), e_src.reshape(16), k_src.reshape(9),
                               torch.inverse(k_src).reshape(9), torch.inverse(e_src).reshape(16), e_ref.reshape(16),
                               k_ref.reshape(9)]))
    return torch.stack(rows).contiguous()


def fuse_view(ref_depth: torch.Tensor, ref_conf: torch.Tensor, ref_cam: torch.Tensor, src_depths: torch.Tensor,
              src_confs: torch.Tensor, src_cams: torch.Tensor, conf: Sequence[float] = (0.0, 0.0, 0.0),
              thres_disp: float = 1.0, thres_view: int = 3, want_view_masks: bool = False) -> Dict[str, torch.Tensor]:
    """One reference view: device tensors ref_depth [h,w], ref_conf [3,h,w], src_depths [V,h,w], src_confs [V,3,h,w];
    cameras ref_cam [2,4,4], src_cams [V,2,4,4] (any device; they are inverted on the host)."""
    dev = ref_depth.device
    cams = camera_chains(ref_cam, src_cams).to(dev)
    fused, mask, points, vm = ops.depth_fusion(ref_depth.contiguous(), ref_conf.contiguous(), src_depths.contiguous(),
                                               src_confs.contiguous(), cams, conf, thres_disp, 0.01, thres_view,
                                               want_view_masks)
    return {"depth": fused, "mask": mask, "points": points, "view_masks": vm}


DYN_DIST_BASE = 0.25            # pixels per level
DYN_REL_BASE = 1.0 / 1300.0     # relative depth difference per level
DYN_VIEWS = (2, 10)             # (n_min, n_max)


def fuse_view_dynamic(ref_depth: torch.Tensor, ref_conf: torch.Tensor, ref_cam: torch.Tensor, src_depths: torch.Tensor,
                      src_confs: torch.Tensor, src_cams: torch.Tensor, conf: Sequence[float] = (0.0, 0.0, 0.0),
                      dist_base: float = DYN_DIST_BASE, rel_base: float = DYN_REL_BASE, n_views: Sequence[int] = DYN_VIEWS,
                      want_admit: bool = False, want_levels: bool = False) -> Dict[str, torch.Tensor]:
    """One reference view with the dynamic consistency check; tensors as :func:`fuse_view`.  With ``want_admit`` the dict
    carries "admit" [h,w] uint8 (the level a pixel was admitted at, 0: not admitted), with ``want_levels`` "levels"
    [V,h,w] uint8 (the level of every view, n_max + 1: inconsistent)."""
    dev = ref_depth.device
    cams = camera_chains(ref_cam, src_cams).to(dev)
    fused, mask, points, admit, levels = ops.depth_fusion_dynamic(
        ref_depth.contiguous(), ref_conf.contiguous(), src_depths.contiguous(), src_confs.contiguous(), cams, conf, dist_base,
        rel_base, n_views, want_admit, want_levels)
    out = {"depth": fused, "mask": mask, "points": points}
    if want_admit:
        out["admit"] = admit
    if want_levels:
        out["levels"] = levels
    return out


def filter_depth(pair_folder: str, scan_folder: str, plyfilename: str, conf: Sequence[float] = (0.0, 0.0, 0.0),
                 thres_disp: float = 1.0, thres_view: int = 3, n_src_views: int = 10, device: str = "cuda",
                 verbose: bool = False, method: str = "normal", dist_base: float = DYN_DIST_BASE,
                 rel_base: float = DYN_REL_BASE, n_views: Sequence[int] = DYN_VIEWS, normals: bool = False,
                 normal_radius: int = 2, normal_jump: float = 0.01, normal_min_pts: int = 6,
                 merge_voxel: Optional[float] = None, merge_min_points: int = 1,
                 collect: Optional[List[dict]] = None, outlier_nb: int = 0, outlier_std: float = 2.0,
                 outlier_radius: float = 0.0, outlier_min_nb: int = 0,
                 outlier_max_dist: Optional[float] = None) -> Dict[str, float]:
    """The reference's ``filter_depth`` for one scan: -> PLY at ``plyfilename`` and mean photo/geo/final mask rates.
    ``method="dynamic"`` fuses with :func:`fuse_view_dynamic` (``conf``, ``dist_base``, ``rel_base``, ``n_views``;
    ``thres_disp`` / ``thres_view`` are not used) and also returns ``admitted_at``: {n: share of the reference pixels
    admitted at level n}, averaged over the reference views (their sum is the geometric mask rate).

    ``normals``: every point carries the normal of its reference view's ``depth_est`` map (:func:`ops.depth_normals` with
    ``normal_radius`` / ``normal_jump`` / ``normal_min_pts``; only pixels whose three confidences exceed ``conf`` enter a fit).
    A kept pixel without a normal is dropped; ``no_normal`` is the dropped share of the otherwise kept pixels of the scan
    (``mean_final_mask`` still describes the fusion mask, before that).  ``merge_voxel``: the scan's points are merged to one per
    occupied voxel of that side (:func:`pointcloud.merge_voxels`), voxels with fewer than ``merge_min_points`` points dropped;
    ``points`` then counts the merged cloud and ``merged_from`` the points that went in.

    Whatever the options, a view leaves its kept points, uint8 colours, normals and three counts (kept, kept with a normal,
    pixels) on the device, and the scan is finished once (:func:`_finish_cloud`): 15 bytes per kept point stay there until
    then, a few GB for the largest scenes.  ``mean_final_mask`` is ``mean(kept / pixels)`` over the reference views in
    float64; ``verbose`` prints one line per reference view at the end of the scan.

    ``outlier_nb`` > 0 and / or ``outlier_radius`` > 0 (with ``outlier_std``, ``outlier_min_nb``, ``outlier_max_dist``): the
    cloud goes through :func:`pointcloud.remove_outliers` on the device before it is written, after the voxel
    merge when both are asked for; colours and normals follow the mask, ``points`` counts what is written and the keys of
    ``remove_outliers``'s ``info`` are added, with ``outliers_removed``.  It cleans the written cloud only: with
    ``plyfilename`` None it is a ValueError, and what ``collect`` receives is never filtered.

    ``collect``: a list that receives, per reference view and in ``pair.txt`` order, what a later stage needs of the same pass
    (:func:`cds_mvsnet_amd.mesh.mesh_scan`), all on the device: {"depth" [h,w] the fused depth, "mask" bool [h,w] the
    fusion mask, "image" uint8 [h,w,3], "cam" [2,4,4] (CPU), "points" [k,3] the kept world points, "conf" [h,w] the view's
    last-stage confidence map, the one of the depth map itself}.  The cloud is written as
    without it; ``plyfilename`` may then be None, and no cloud is written."""
    if method not in ("normal", "dynamic"):
        raise ValueError(f"filter_depth: method must be 'normal' or 'dynamic', got {method!r}")
    if plyfilename is None and collect is None:
        raise ValueError("filter_depth: plyfilename is None and nothing is collected")
    from .pointcloud import check_outlier_args
    check_outlier_args(outlier_nb, outlier_std, outlier_radius, outlier_min_nb, outlier_max_dist)
    outliers = dict(nb_neighbors=outlier_nb, std_ratio=outlier_std, radius=outlier_radius, min_neighbors=outlier_min_nb,
                    max_dist=outlier_max_dist) if outlier_nb > 0 or outlier_radius > 0 else None
    if outliers is not None and plyfilename is None:
        raise ValueError("filter_depth: the outlier removal cleans the cloud that is written; plyfilename is None")
    if merge_voxel is not None and not (float(merge_voxel) > 0 and np.isfinite(float(merge_voxel))):
        raise ValueError(f"filter_depth: merge_voxel must be positive, got {merge_voxel}")
    pairs = read_pair_file(os.path.join(pair_folder, "pair.txt"))
    scan = ScanFolder(scan_folder)
    cache: Dict[int, tuple] = {}

    def view(vid):
        if vid not in cache:
            cache[vid] = (torch.from_numpy(scan.depth(vid)).to(device), torch.from_numpy(scan.conf(vid)).to(device),
                          torch.from_numpy(scan.cam(vid)))
        return cache[vid]

    fused: List[tuple] = []     # per reference view: (id, points [k,3], colours uint8 [k,3], normals [k,3] | None, counts [3])
    hist: List[torch.Tensor] = []
    for ref, srcs in pairs:
        srcs = srcs[:n_src_views]
        if not srcs:
            continue
        rd, rc, rcam = view(ref)
        sd, sc, scam = (torch.stack(a) for a in zip(*(view(s) for s in srcs)))
        if method == "dynamic":
            out = fuse_view_dynamic(rd, rc, rcam, sd, sc, scam, conf, dist_base, rel_base, n_views, want_admit=True)
            hist.append(torch.bincount(out["admit"].reshape(-1).long(), minlength=int(n_views[1]) + 1))
        else:
            out = fuse_view(rd, rc, rcam, sd, sc, scam, conf, thres_disp, thres_view)
        keep = out["mask"] > 0.5
        img = torch.from_numpy(scan.image(ref)).to(device)                          # uint8 [h,w,3]
        if collect is not None:
            collect.append({"depth": out["depth"], "mask": keep, "image": img, "cam": rcam,
                            "points": out["points"][:, keep].t().contiguous(), "conf": rc[-1]})
        kept, nrm = keep.sum(), None
        if normals:
            th = torch.tensor([float(c) for c in conf], dtype=torch.float32, device=rc.device).view(3, 1, 1)
            nrm, ok = ops.depth_normals(rd, rcam[1, :3, :3], rcam[0], valid=(rc > th).all(0), radius=normal_radius,
                                        jump=normal_jump, min_pts=normal_min_pts)
            keep = keep & (ok > 0)
            nrm = nrm[:, keep].t().contiguous()
        counts = torch.stack([kept, keep.sum(), kept.new_full((), keep.numel())])      # kept, kept with a normal, pixels
        fused.append((ref, out["points"][:, keep].t().contiguous(), img[keep], nrm, counts))
    info = _finish_cloud(plyfilename, fused, bool(normals), merge_voxel, merge_min_points, device, verbose, scan_folder, outliers)
    if method == "dynamic":
        pixels = torch.stack([f[4][2] for f in fused]).cpu().numpy().astype(np.float64) if fused else None
        share = np.mean(torch.stack(hist).cpu().numpy() / pixels[:, None], 0) if hist else np.zeros(int(n_views[1]) + 1)
        info["admitted_at"] = {n: float(share[n]) for n in range(int(n_views[0]), int(n_views[1]) + 1)}
    return info


def _finish_cloud(plyfilename, fused, normals, merge_voxel, merge_min_points, device, verbose, scan_folder,
                  outliers=None) -> Dict[str, float]:
    """The end of a scan in :func:`filter_depth`.  ``fused``: per reference view (id, points, colours, normals | None, counts),
    on the device.  One read-back of the counts gives ``points`` and ``mean_final_mask``; with a ``plyfilename`` the views are
    concatenated, merged once, cleaned of outliers (``outliers``: the keyword arguments of :func:`pointcloud.remove_outliers`,
    or None), downloaded once and written."""
    from .pointcloud import merge_voxels
    cnt = torch.stack([f[4] for f in fused]).cpu().numpy().astype(np.float64) if fused else np.zeros((0, 3))
    if verbose:
        for (ref, *_), (k, with_n, px) in zip(fused, cnt):
            print(f"processing {scan_folder}, ref-view{ref:02d}, final-mask:{k / px:.4f}"
                  + (f", with a normal:{with_n / px:.4f}" if normals else ""))
    info = {"points": int(cnt[:, 1].sum()), "mean_final_mask": float(np.mean(cnt[:, 0] / cnt[:, 2])) if len(cnt) else 0.0}
    if plyfilename is None:
        return info
    def cat(i, dtype):
        return torch.cat([f[i] for f in fused]) if fused else torch.zeros((0, 3), dtype=dtype, device=device)

    pts, col, nrm = cat(1, torch.float32), cat(2, torch.uint8), cat(3, torch.float32) if normals else None
    if normals:
        kept = float(cnt[:, 0].sum())
        info["no_normal"] = float((kept - cnt[:, 1].sum()) / kept) if kept > 0 else 0.0
    if merge_voxel is not None:
        m = merge_voxels(pts, col, float(merge_voxel), normals=nrm, min_points=merge_min_points)
        info["merged_from"] = info["points"]
        pts, col, nrm = m["points"], m["colors"], m["normals"]
        info["points"] = int(pts.shape[0])
    if outliers is not None:
        pts, col, nrm = clean_cloud(pts, col, nrm, outliers, info)
    write_ply(plyfilename, pts.cpu().numpy(), col.cpu().numpy(), None if nrm is None else nrm.cpu().numpy())
    return info


def clean_cloud(pts, col, nrm, outliers: dict, info: dict):
    """:func:`pointcloud.remove_outliers` with the keyword arguments ``outliers`` on a cloud on the device (points [N,3],
    colours, normals or None) -> what stays, rows in input order and bit for bit; ``info`` receives the filter's figures,
    ``outliers_removed`` and the new ``points``."""
    from .pointcloud import remove_outliers
    keep = remove_outliers(pts, info=info, **outliers)
    info["outliers_removed"] = int(pts.shape[0]) - int(keep.sum())
    info["points"] = int(pts.shape[0]) - info["outliers_removed"]
    return pts[keep], col[keep], None if nrm is None else nrm[keep]


# --------------------------------------------------------------------------------------------------------------- CLI
def add_cloud_args(ap: argparse.ArgumentParser, normals: bool = True) -> None:
    """The options of DESIGN §1.8, shared by the fusion command lines (gipuma takes the merge only)."""
    if normals:
        ap.add_argument("--normals", action="store_true",
                        help="write nx ny nz: the oriented normal of each point, from its reference view's depth map")
        ap.add_argument("--normal_radius", type=int, default=2, help="normals: window radius in pixels, 1..4")
        ap.add_argument("--normal_jump", type=float, default=0.01,
                        help="normals: a neighbour enters the fit when its depth is within this share of the centre's")
        ap.add_argument("--normal_min_pts", type=int, default=6, help="normals: pixels a fit needs, 3..(2 radius + 1)^2")
    ap.add_argument("--merge_voxel", type=float, default=None, metavar="SIZE",
                    help="merge the fused cloud to one point per occupied voxel of this side (world units)")
    ap.add_argument("--merge_min_points", type=int, default=1, metavar="K",
                    help="--merge_voxel: drop voxels with fewer than K points")


def cloud_kwargs(args: argparse.Namespace) -> dict:
    """The arguments of :func:`add_cloud_args` as keyword arguments of :func:`filter_depth`."""
    return dict(normals=args.normals, normal_radius=args.normal_radius, normal_jump=args.normal_jump,
                normal_min_pts=args.normal_min_pts, merge_voxel=args.merge_voxel, merge_min_points=args.merge_min_points)


def format_cloud(info: Dict[str, float]) -> str:
    """", no normal 1.2%, merged from 25700000" for the keys the options of DESIGN §1.8 add; "" without them."""
    text = f", no normal {100.0 * info['no_normal']:.1f}%" if "no_normal" in info else ""
    return text + (f", merged from {info['merged_from']}" if "merged_from" in info else "")


def add_outlier_args(ap: argparse.ArgumentParser) -> None:
    """The options of DESIGN §1.16, shared by the fusion command lines."""
    ap.add_argument("--outlier_nb", type=int, default=0, metavar="K",
                    help="statistical outlier removal: drop a point whose mean distance to its K nearest neighbours exceeds "
                         "the cloud's mean + --outlier_std standard deviations (0 = off, at most 63)")
    ap.add_argument("--outlier_std", type=float, default=2.0, metavar="R", help="--outlier_nb: the multiple of the deviation")
    ap.add_argument("--outlier_radius", type=float, default=0.0, metavar="r",
                    help="radius outlier removal: drop a point with fewer than --outlier_min_nb others within r (0 = off)")
    ap.add_argument("--outlier_min_nb", type=int, default=0, metavar="n", help="--outlier_radius: neighbours a point needs")
    ap.add_argument("--outlier_max_dist", type=float, default=None, metavar="d",
                    help="--outlier_nb: cap on every neighbour distance (default: 16 cells of the search grid)")


def outlier_kwargs(args: argparse.Namespace, ap: Optional[argparse.ArgumentParser] = None) -> dict:
    """The arguments of :func:`add_outlier_args` as keyword arguments of :func:`filter_depth` / ``gipuma.filter_scan``.  With
    ``ap``, a bad combination ends the program through ``ap.error`` (status 2) with a message that names the flag."""
    if ap is not None:
        from .pointcloud import KNN_MAX_K
        if not 0 <= args.outlier_nb <= KNN_MAX_K - 1:
            ap.error(f"--outlier_nb must be in 0..{KNN_MAX_K - 1}, got {args.outlier_nb}")
        if not (args.outlier_std >= 0 and np.isfinite(args.outlier_std)):
            ap.error(f"--outlier_std must be finite and >= 0, got {args.outlier_std}")
        if not (args.outlier_radius >= 0 and np.isfinite(args.outlier_radius)):
            ap.error(f"--outlier_radius must be finite and >= 0, got {args.outlier_radius}")
        if args.outlier_min_nb < 0:
            ap.error(f"--outlier_min_nb must be >= 0, got {args.outlier_min_nb}")
        if args.outlier_radius > 0 and args.outlier_min_nb < 1:
            ap.error("--outlier_radius needs --outlier_min_nb >= 1")
        if args.outlier_min_nb > 0 and not args.outlier_radius > 0:
            ap.error("--outlier_min_nb belongs to --outlier_radius")
        if args.outlier_max_dist is not None and not args.outlier_max_dist > 0:
            ap.error(f"--outlier_max_dist must be positive, got {args.outlier_max_dist}")
        if args.outlier_max_dist is not None and args.outlier_nb == 0:
            ap.error("--outlier_max_dist belongs to --outlier_nb")
    return dict(outlier_nb=args.outlier_nb, outlier_std=args.outlier_std, outlier_radius=args.outlier_radius,
                outlier_min_nb=args.outlier_min_nb, outlier_max_dist=args.outlier_max_dist)


def format_outliers(info: Dict[str, float]) -> str:
    """", outliers removed 1234 (threshold 0.00321)" for the keys the options of DESIGN §1.16 add; "" without them."""
    if "outliers_removed" not in info:
        return ""
    t = info.get("threshold")
    return f", outliers removed {info['outliers_removed']}" + (f" (threshold {t:.6g})" if t is not None else "")


def clean_ply(src: str, dst: str, device: str = "cuda", **outliers) -> Dict[str, float]:
    """Re-clean a saved cloud without the fusion: :func:`read_ply_full` -> :func:`pointcloud.remove_outliers` (keyword
    arguments ``outliers``) -> :func:`write_ply`, normals kept when present.  -> {"points", "outliers_removed", mu, ...}."""
    p, c, nrm = read_ply_full(src)
    info: Dict[str, float] = {}
    pts, col, nrm = clean_cloud(torch.from_numpy(np.ascontiguousarray(p)).to(device), torch.from_numpy(np.ascontiguousarray(c)).to(device),
                                None if nrm is None else torch.from_numpy(np.ascontiguousarray(nrm)).to(device), outliers, info)
    write_ply(dst, pts.cpu().numpy(), col.cpu().numpy(), None if nrm is None else nrm.cpu().numpy())
    return info


def _floats(text: str, n: int, what: str) -> List[float]:
    vals = [float(v) for v in text.split(",")]
    if len(vals) != n:
        raise ValueError(f"{what}: {n} comma-separated numbers expected, got {text!r}")
    return vals


def format_admitted(admitted_at: Dict[int, float]) -> str:
    """"n=2 31.0% n=3 4.2% ..." for the levels that admitted any pixel."""
    return " ".join(f"n={n} {100.0 * s:.1f}%" for n, s in admitted_at.items() if s > 0) or "none"


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--testpath", default=None, help="the scenes: <testpath>/<scan>/pair.txt (not needed with --from_ply)")
    ap.add_argument("--outdir", required=True, help="the infer output folder: <outdir>/<scan>/{depth_est,confidence,cams,images}")
    ap.add_argument("--testlist", required=True, help="text file with one scan name per line")
    ap.add_argument("--filter_method", default="normal", choices=["normal", "dynamic"])
    ap.add_argument("--conf", default="0.0,0.0,0.0", help="per-stage confidence thresholds")
    ap.add_argument("--thres_view", type=int, default=3, help="normal: consistent views a pixel needs")
    ap.add_argument("--thres_disp", type=float, default=1.0, help="normal: re-projection distance threshold in pixels")
    ap.add_argument("--dyn_dist_base", type=float, default=DYN_DIST_BASE, help="dynamic: pixels per level")
    ap.add_argument("--dyn_rel_base", type=float, default=DYN_REL_BASE, help="dynamic: relative depth difference per level")
    ap.add_argument("--dyn_views", default="2,10", help="dynamic: n_min,n_max")
    ap.add_argument("--device", default="cuda")
    add_cloud_args(ap)
    add_outlier_args(ap)
    ap.add_argument("--from_ply", default=None, metavar="PATTERN",
                    help="no fusion: read the saved cloud PATTERN with {scan} filled in, remove its outliers (--outlier_*) and write "
                         "<outdir>/<scan>.ply (normals kept when the file has them)")
    args = ap.parse_args(argv)
    args.outliers = outlier_kwargs(args, ap)
    if args.from_ply is not None and not (args.outlier_nb > 0 or args.outlier_radius > 0):
        ap.error("--from_ply removes outliers from a saved cloud: give --outlier_nb and / or --outlier_radius")
    if args.from_ply is None and args.testpath is None:
        ap.error("--testpath is required (without --from_ply)")
    args.conf = _floats(args.conf, 3, "--conf")
    args.dyn_views = tuple(int(v) for v in _floats(args.dyn_views, 2, "--dyn_views"))
    return args


def main(argv=None) -> Dict[str, Dict[str, float]]:
    args = parse_args(argv)
    out = {}
    for scan in read_testlist(args.testlist):
        if args.from_ply is not None:
            o = args.outliers
            os.makedirs(args.outdir, exist_ok=True)
            info = clean_ply(args.from_ply.format(scan=scan), os.path.join(args.outdir, f"{scan}.ply"), args.device,
                             nb_neighbors=o["outlier_nb"], std_ratio=o["outlier_std"], radius=o["outlier_radius"],
                             min_neighbors=o["outlier_min_nb"], max_dist=o["outlier_max_dist"])
            out[scan] = info
            print(f"{scan}.ply: {info['points']} points{format_outliers(info)}", flush=True)
            continue
        info = filter_depth(os.path.join(args.testpath, scan), os.path.join(args.outdir, scan),
                            os.path.join(args.outdir, f"{scan}.ply"), conf=args.conf, thres_disp=args.thres_disp,
                            thres_view=args.thres_view, device=args.device, method=args.filter_method,
                            dist_base=args.dyn_dist_base, rel_base=args.dyn_rel_base, n_views=args.dyn_views,
                            **cloud_kwargs(args), **args.outliers)
        out[scan] = info
        extra = f", admitted at {format_admitted(info['admitted_at'])}" if "admitted_at" in info else ""
        extra += format_cloud(info) + format_outliers(info)
        print(f"{scan}.ply: {info['points']} points, final mask {info['mean_final_mask']:.3f}{extra}", flush=True)
    return out


if __name__ == "__main__":
    main()
