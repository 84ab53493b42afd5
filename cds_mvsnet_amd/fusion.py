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

re-fuses saved depth maps (``<out>/<scan>/``, pairs from ``<scenes>/<scan>/pair.txt``) into ``<out>/<scan>.ply`` without
running the network again.
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .mvs_io import read_pair_file, read_pfm


def read_fusion_cam(path: str) -> np.ndarray:
    """``cams/%08d_cam.txt`` as written by save_outputs -> [2,4,4] (extrinsic; intrinsic in [:3,:3], [3,3]=1)
    (test.py:85-95, 285-288)."""
    with open(path) as f:
        lines = [ln.rstrip() for ln in f.readlines()]
    cam = np.zeros((2, 4, 4), dtype=np.float32)
    cam[0] = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape(4, 4)
    cam[1, :3, :3] = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape(3, 3)
    cam[1, 3, 3] = 1.0
    return cam


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


def write_ply(path: str, points: np.ndarray, colors: np.ndarray) -> None:
    """Binary little-endian PLY with x,y,z float32 + red,green,blue uint8 vertices (what plyfile writes in
    test.py:370-382)."""
    n = int(points.shape[0])
    rec = np.empty(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = points[:, 0], points[:, 1], points[:, 2]
    rec["red"], rec["green"], rec["blue"] = colors[:, 0], colors[:, 1], colors[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\n" f"element vertex {n}\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        rec.tofile(f)


def read_ply(path: str) -> Tuple[np.ndarray, np.ndarray]:
    with open(path, "rb") as f:
        n = None
        while True:
            line = f.readline().decode("ascii").strip()
            if line.startswith("element vertex"):
                n = int(line.split()[-1])
            if line == "end_header":
                break
        rec = np.frombuffer(f.read(), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"),
                                             ("blue", "u1")], count=n)
    return np.stack([rec["x"], rec["y"], rec["z"]], -1), np.stack([rec["red"], rec["green"], rec["blue"]], -1)


def _load_view(scan_folder: str, vid: int):
    from PIL import Image
    depth = read_pfm(os.path.join(scan_folder, "depth_est", f"{vid:08d}.pfm"))[0]
    conf = read_pfm(os.path.join(scan_folder, "confidence", f"{vid:08d}.pfm"))[0]
    cam = read_fusion_cam(os.path.join(scan_folder, "cams", f"{vid:08d}_cam.txt"))
    return np.ascontiguousarray(depth, dtype=np.float32), np.ascontiguousarray(conf.transpose(2, 0, 1)), cam, \
        lambda: np.asarray(Image.open(os.path.join(scan_folder, "images", f"{vid:08d}.jpg")), dtype=np.float32) / 255.0


def filter_depth(pair_folder: str, scan_folder: str, plyfilename: str, conf: Sequence[float] = (0.0, 0.0, 0.0),
                 thres_disp: float = 1.0, thres_view: int = 3, n_src_views: int = 10, device: str = "cuda",
                 verbose: bool = False, method: str = "normal", dist_base: float = DYN_DIST_BASE,
                 rel_base: float = DYN_REL_BASE, n_views: Sequence[int] = DYN_VIEWS) -> Dict[str, float]:
    """The reference's ``filter_depth`` for one scan: -> PLY at ``plyfilename`` and mean photo/geo/final mask rates.
    ``method="dynamic"`` fuses with :func:`fuse_view_dynamic` (``conf``, ``dist_base``, ``rel_base``, ``n_views``;
    ``thres_disp`` / ``thres_view`` are not used) and also returns ``admitted_at``: {n: share of the reference pixels
    admitted at level n}, averaged over the reference views (their sum is the geometric mask rate)."""
    if method not in ("normal", "dynamic"):
        raise ValueError(f"filter_depth: method must be 'normal' or 'dynamic', got {method!r}")
    pairs = read_pair_file(os.path.join(pair_folder, "pair.txt"))
    cache: Dict[int, tuple] = {}

    def view(vid):
        if vid not in cache:
            d, c, cam, img = _load_view(scan_folder, vid)
            cache[vid] = (torch.from_numpy(d).to(device), torch.from_numpy(c).to(device), torch.from_numpy(cam), img)
        return cache[vid]

    pts_all: List[np.ndarray] = []
    col_all: List[np.ndarray] = []
    rates = []
    hist: List[np.ndarray] = []
    for ref, srcs in pairs:
        srcs = srcs[:n_src_views]
        if not srcs:
            continue
        rd, rc, rcam, rimg = view(ref)
        sv = [view(s) for s in srcs]
        if method == "dynamic":
            out = fuse_view_dynamic(rd, rc, rcam, torch.stack([s[0] for s in sv]), torch.stack([s[1] for s in sv]),
                                    torch.stack([s[2] for s in sv]), conf, dist_base, rel_base, n_views, want_admit=True)
            # one read-back per view: how many pixels were admitted at each level
            hist.append(torch.bincount(out["admit"].reshape(-1).long(), minlength=int(n_views[1]) + 1).cpu().numpy()
                        / float(out["admit"].numel()))
        else:
            out = fuse_view(rd, rc, rcam, torch.stack([s[0] for s in sv]), torch.stack([s[1] for s in sv]),
                            torch.stack([s[2] for s in sv]), conf, thres_disp, thres_view)
        keep = out["mask"] > 0.5
        pts = out["points"][:, keep].t().contiguous().cpu().numpy()
        img = torch.from_numpy(np.ascontiguousarray(rimg())).to(device)            # [h,w,3]
        col = (img[keep] * 255).to(torch.uint8).cpu().numpy()
        pts_all.append(pts)
        col_all.append(col)
        rates.append(float(keep.float().mean()))
        if verbose:
            print(f"processing {scan_folder}, ref-view{ref:02d}, final-mask:{rates[-1]:.4f}")
    p_all = np.concatenate(pts_all, 0) if pts_all else np.zeros((0, 3), np.float32)
    c_all = np.concatenate(col_all, 0) if col_all else np.zeros((0, 3), np.uint8)
    write_ply(plyfilename, p_all, c_all)
    info = {"points": int(p_all.shape[0]), "mean_final_mask": float(np.mean(rates)) if rates else 0.0}
    if method == "dynamic":
        share = np.mean(hist, 0) if hist else np.zeros(int(n_views[1]) + 1)
        info["admitted_at"] = {n: float(share[n]) for n in range(int(n_views[0]), int(n_views[1]) + 1)}
    return info


# --------------------------------------------------------------------------------------------------------------- CLI
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
    ap.add_argument("--testpath", required=True, help="the scenes: <testpath>/<scan>/pair.txt")
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
    args = ap.parse_args(argv)
    args.conf = _floats(args.conf, 3, "--conf")
    args.dyn_views = tuple(int(v) for v in _floats(args.dyn_views, 2, "--dyn_views"))
    return args


def main(argv=None) -> Dict[str, Dict[str, float]]:
    args = parse_args(argv)
    with open(args.testlist) as f:
        scans = [ln.strip() for ln in f if ln.strip()]
    out = {}
    for scan in scans:
        info = filter_depth(os.path.join(args.testpath, scan), os.path.join(args.outdir, scan),
                            os.path.join(args.outdir, f"{scan}.ply"), conf=args.conf, thres_disp=args.thres_disp,
                            thres_view=args.thres_view, device=args.device, method=args.filter_method,
                            dist_base=args.dyn_dist_base, rel_base=args.dyn_rel_base, n_views=args.dyn_views)
        out[scan] = info
        extra = f", admitted at {format_admitted(info['admitted_at'])}" if "admitted_at" in info else ""
        print(f"{scan}.ply: {info['points']} points, final mask {info['mean_final_mask']:.3f}{extra}", flush=True)
    return out


if __name__ == "__main__":
    main()
