"""A triangle mesh rendered into the views of a scan, on the GPU: depth maps, pseudo ground truth (the rule is in
include/cds_mvsnet_hip.h).

Per view and pixel: the nearest depth of the mesh along the pixel's ray, the face it came from, whether that face looks at the
camera, and the interpolated vertex colour.  The output is a function of the input alone: integer coverage with a top-left rule
on coordinates snapped to 1/256 pixel, depth from the face's plane in fp64, and a 64-bit minimum over (depth bits, face index).
The hot paths are the kernels of ``csrc/raster.hip`` (``cds_raster_project``, ``cds_raster_faces``, ``cds_raster_large``,
``cds_raster_resolve``); torch lists the large faces between two launches.  There is no CPU path.

    python -m cds_mvsnet_amd.render --testpath <scenes> --outdir <out> --testlist <list> [--mesh "<out>/{scan}_mesh.ply"]
        [--back mask|keep] [--max_rel_diff R] [--export_blended DIR] [--save_image]

renders ``<out>/<scan>_mesh.ply`` (``python -m cds_mvsnet_amd.mesh``, ``infer --fuse --mesh_voxel``) into every view of
``<testpath>/<scan>/pair.txt`` with the cameras of ``<out>/<scan>/cams`` and writes ``<out>/<scan>/depth_mesh/%08d.pfm``.
``--export_blended DIR`` also writes the tree ``fit --dataset blended --datapath DIR --crop H,W`` trains from.
``infer ... --fuse --mesh_voxel SIZE --render_mesh`` does the same right after the mesh is written.
"""
from __future__ import annotations

import argparse
import os
import shutil
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import check
from .mesh import check_mesh_device, check_mesh_layout, load_mesh
from .mvs_io import ScanFolder, read_pair_file, read_testlist, write_pfm

Tensor = torch.Tensor

MAX_CHUNK = 32                 # views per launch the kernels take (CDS_RASTER_MAX_CHUNK)
CAM_DOUBLES = 24               # CDS_RASTER_CAM
MAX_LIST = 1 << 30             # entries of one cds_raster_large launch (CDS_RASTER_MAX_LIST)
OUTPUTS = (("depth", torch.float32), ("face", torch.int32), ("front", torch.uint8), ("valid", torch.uint8))


def camera_table(cams: Tensor) -> Tensor:
    """cams [V,2,4,4] (extrinsic; K in [:3,:3]) -> the kernels' table, float64 [V,24] on the host.  ValueError unless every K is
    [[fx, s, cx], [0, fy, cy], [0, 0, 1]]."""
    cam = cams.detach().to(torch.float32).cpu().double()
    K = cam[:, 1, :3, :3]
    bad = (K[:, 1, 0] != 0) | (K[:, 2, 0] != 0) | (K[:, 2, 1] != 0) | (K[:, 2, 2] != 1)
    if bool(bad.any()):
        v = int(torch.nonzero(bad)[0])
        raise ValueError(f"render_mesh: the intrinsic of view {v} must be [[fx, s, cx], [0, fy, cy], [0, 0, 1]], got {K[v].tolist()}")
    tab = torch.zeros((cam.shape[0], CAM_DOUBLES), dtype=torch.float64)
    tab[:, 0:9] = cam[:, 0, :3, :3].reshape(-1, 9)
    tab[:, 9:12] = cam[:, 0, :3, 3]
    tab[:, 12], tab[:, 13], tab[:, 14], tab[:, 15], tab[:, 16] = K[:, 0, 0], K[:, 0, 1], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2]
    return tab


def large_list(large: Tensor) -> Tensor:
    """The class bytes [n,NF] of cds_raster_faces -> the entries view * NF + face of cds_raster_large, int64, ascending.  A scan's
    own mesh has sub-pixel faces and usually none is large: one reduction finds that out at a fifth of the cost of the compaction
    (profiles/render_mesh.md: 2.0 against 9.2 ms over a scan)."""
    flat = large.reshape(-1)
    if not bool(flat.any()):
        return torch.zeros(0, dtype=torch.int64, device=large.device)
    return torch.nonzero(flat).reshape(-1)


def render_mesh(vertices: Tensor, faces: Tensor, cams: Tensor, h: int, w: int, colors: Optional[Tensor] = None, chunk: int = 8,
                large_px: int = 64) -> Dict[str, Tensor]:
    """vertices float32 [NV,3], faces int32 [NF,3], optional colors uint8 [NV,3], all on one ROCm device; cams [V,2,4,4] on any
    device -> {"depth" float32, "face" int32, "front" uint8, "valid" uint8 [V,h,w][, "image" uint8 [V,h,w,3]]} on that device.
    ``chunk`` views go into one launch (1..32); a face with more than ``large_px`` candidate pixels is drawn by a wave instead of
    a thread.  The result depends on neither.  The mesh is checked as the mesh stage checks it (mesh.check_mesh_layout, then the
    arguments of this function, then mesh.check_mesh_device)."""
    what = "render_mesh"
    nv_mesh, nf = check_mesh_layout(vertices, colors, faces, what), int(faces.shape[0])
    if not isinstance(cams, torch.Tensor) or cams.dim() != 4 or tuple(cams.shape[1:]) != (2, 4, 4):
        raise ValueError(f"{what}: cams must be [V,2,4,4], got {tuple(getattr(cams, 'shape', ()))}")
    h, w, chunk, large_px = int(h), int(w), int(chunk), int(large_px)
    if h < 1 or w < 1 or h * w >= 2 ** 31:
        raise ValueError(f"{what}: a map of {h} x {w}")
    if not (1 <= chunk <= MAX_CHUNK):
        raise ValueError(f"{what}: chunk must lie in 1..{MAX_CHUNK}, got {chunk}")
    if large_px < 1:
        raise ValueError(f"{what}: large_px must be >= 1, got {large_px}")
    tab = camera_table(cams)
    dev = check_mesh_device(vertices, colors, faces, what)
    v = int(tab.shape[0])
    out = {name: torch.zeros((v, h, w), dtype=dt, device=dev) for name, dt in OUTPUTS}
    out["face"].fill_(-1)
    if colors is not None:
        out["image"] = torch.zeros((v, h, w, 3), dtype=torch.uint8, device=dev)
    if v == 0 or nf == 0:
        return out
    vertices, faces = vertices.contiguous(), faces.contiguous()
    colors = colors.contiguous() if colors is not None else None
    tab = tab.to(dev)
    lib, hw = _lib.load(), h * w
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        n = min(chunk, v)
        xy = torch.empty((n, nv_mesh, 2), dtype=torch.int32, device=dev)
        xc = torch.empty((n, nv_mesh, 3), dtype=torch.float64, device=dev)
        keys = torch.empty((n, h, w), dtype=torch.int64, device=dev)
        large = torch.empty((n, nf), dtype=torch.uint8, device=dev)
        for v0 in range(0, v, chunk):
            n = min(chunk, v - v0)
            cam = tab.data_ptr() + 8 * CAM_DOUBLES * v0
            keys.fill_(-1)                                             # all ones
            check(lib.cds_raster_project(vertices.data_ptr(), nv_mesh, cam, n, xy.data_ptr(), xc.data_ptr(), stream),
                  "cds_raster_project")
            check(lib.cds_raster_faces(faces.data_ptr(), nf, nv_mesh, cam, n, xy.data_ptr(), xc.data_ptr(), h, w, large_px,
                                       keys.data_ptr(), large.data_ptr(), stream), "cds_raster_faces")
            todo = large_list(large[:n])
            for l0 in range(0, int(todo.numel()), MAX_LIST):
                part = todo[l0:l0 + MAX_LIST]
                check(lib.cds_raster_large(part.data_ptr(), int(part.numel()), faces.data_ptr(), nf, nv_mesh, cam, n, xy.data_ptr(),
                                           xc.data_ptr(), h, w, keys.data_ptr(), stream), "cds_raster_large")
            check(lib.cds_raster_resolve(keys.data_ptr(), faces.data_ptr(), nf, nv_mesh, cam, n, xc.data_ptr(),
                                         colors.data_ptr() if colors is not None else None, h, w,
                                         out["depth"].data_ptr() + 4 * v0 * hw, out["face"].data_ptr() + 4 * v0 * hw,
                                         out["front"].data_ptr() + v0 * hw, out["valid"].data_ptr() + v0 * hw,
                                         out["image"].data_ptr() + 3 * v0 * hw if colors is not None else None, stream),
                  "cds_raster_resolve")
    return out


# -------------------------------------------------------------------------------------------------------------------- scans
def render_scan(scan_out_folder: str, mesh_ply, pair_folder: str, subdir: str = "depth_mesh", back: str = "mask",
                max_rel_diff: Optional[float] = None, save_image: bool = False, device: str = "cuda", chunk: int = 8,
                large_px: int = 64) -> Dict[str, object]:
    """Render a mesh into every view of ``<pair_folder>/pair.txt``, in that order, with the cameras of
    ``<scan_out_folder>/cams/%08d_cam.txt`` and the map size of ``depth_est/%08d.pfm``, and write
    ``<scan_out_folder>/<subdir>/%08d.pfm``: the depth where the nearest face looks at the camera, 0 elsewhere.

    ``mesh_ply``: a file of ``mesh.write_mesh_ply``, or the mesh dict of ``TsdfVolume.extract`` on the device.
    ``back="keep"`` writes the depth of back-facing hits too.  ``max_rel_diff=R`` also zeroes a pixel whose depth_est is > 0 and
    differs from the rendered depth by more than R times the rendered depth (a label is kept only where the
    network's own estimate already agrees with the fused surface).  ``save_image`` writes the colour render as ``%08d.jpg``.
    -> {"views", "valid": share of pixels written, "back": share of pixels whose nearest face looks away}."""
    if back not in ("mask", "keep"):
        raise ValueError(f"render_scan: back must be 'mask' or 'keep', got {back!r}")
    if max_rel_diff is not None and not float(max_rel_diff) >= 0:
        raise ValueError(f"render_scan: max_rel_diff must be >= 0, got {max_rel_diff}")
    dev = torch.device(device)
    mesh = load_mesh(mesh_ply, dev)
    scan = ScanFolder(scan_out_folder)
    vids = [ref for ref, _ in read_pair_file(os.path.join(pair_folder, "pair.txt"))]
    os.makedirs(os.path.join(scan_out_folder, subdir), exist_ok=True)
    n_px = n_valid = n_back = 0
    for (h, w), ids in scan.groups(vids, scan.map_size).items():          # views by map size, each in pair.txt order
        out = render_mesh(mesh["vertices"], mesh["faces"], torch.from_numpy(np.stack([scan.cam(i) for i in ids])), h, w,
                          colors=mesh["colors"] if save_image else None, chunk=chunk, large_px=large_px)
        hit = out["face"] >= 0
        keep = hit if back == "keep" else out["valid"] != 0
        depth = out["depth"]
        if max_rel_diff is not None:
            est = torch.from_numpy(np.stack([scan.depth(i) for i in ids])).to(dev)
            keep = keep & ~((est > 0) & ((depth - est).abs() > float(max_rel_diff) * depth))
        depth = torch.where(keep, depth, torch.zeros_like(depth)).cpu().numpy()
        n_px += hit.numel()
        n_valid += int(keep.sum())
        n_back += int((hit & (out["front"] == 0)).sum())
        image = out["image"].cpu().numpy() if save_image else None
        for k, vid in enumerate(ids):
            write_pfm(os.path.join(scan_out_folder, subdir, f"{vid:08d}.pfm"), depth[k])
            if save_image:
                from PIL import Image
                Image.fromarray(image[k]).save(os.path.join(scan_out_folder, subdir, f"{vid:08d}.jpg"), quality=95)
    info = {"views": len(vids), "valid": n_valid / n_px if n_px else 0.0, "back": n_back / n_px if n_px else 0.0}
    print(f"{os.path.basename(os.path.normpath(scan_out_folder))}/{subdir}: {format_render(info)}", flush=True)
    return info


def format_render(info: Dict[str, object]) -> str:
    return f"{info['views']} views, {100.0 * info['valid']:.2f} % valid, {100.0 * info['back']:.2f} % back-facing"


def export_blended(scan: str, testpath: str, outdir: str, dst: str, subdir: str = "depth_mesh") -> int:
    """The tree ``train_data.BlendedTrainScenes`` reads, for one scan: ``dst/<scan>/blended_images/%08d.jpg`` (the bytes of
    ``<outdir>/<scan>/images``), ``cams/%08d_cam.txt`` (extrinsic and K of ``<outdir>/<scan>/cams``, which hold K at the saved
    image's resolution, and the depth-range line of the scene's own ``<testpath>/<scan>/cams`` file), ``cams/pair.txt`` (the
    scene's) and ``rendered_depth_maps/%08d.pfm`` (``<outdir>/<scan>/<subdir>``).  -> the number of views."""
    src, out = os.path.join(testpath, scan), os.path.join(outdir, scan)
    for sub in ("blended_images", "cams", "rendered_depth_maps"):
        os.makedirs(os.path.join(dst, scan, sub), exist_ok=True)
    vids = [ref for ref, _ in read_pair_file(os.path.join(src, "pair.txt"))]
    for vid in vids:
        name = f"{vid:08d}"
        shutil.copyfile(os.path.join(out, "images", name + ".jpg"), os.path.join(dst, scan, "blended_images", name + ".jpg"))
        shutil.copyfile(os.path.join(out, subdir, name + ".pfm"), os.path.join(dst, scan, "rendered_depth_maps", name + ".pfm"))
        with open(os.path.join(out, "cams", name + "_cam.txt")) as f:
            lines = [ln.rstrip("\n") for ln in f.readlines()]
        with open(os.path.join(src, "cams", name + "_cam.txt")) as f:
            scene = [ln.rstrip() for ln in f.readlines()]
        if len(lines) < 10 or len(scene) < 12 or len(scene[11].split()) < 2:
            raise ValueError(f"export_blended: {scan} view {vid}: a camera file without its matrices or its depth-range line")
        with open(os.path.join(dst, scan, "cams", name + "_cam.txt"), "w") as f:
            f.write("\n".join(lines[:10] + ["", scene[11]]) + "\n")
    shutil.copyfile(os.path.join(src, "pair.txt"), os.path.join(dst, scan, "cams", "pair.txt"))
    return len(vids)


# ---------------------------------------------------------------------------------------------------------------------- CLI
def add_render_args(ap: argparse.ArgumentParser) -> None:
    """The options of DESIGN §1.10 that ``infer --render_mesh`` shares."""
    ap.add_argument("--back", default="mask", choices=["mask", "keep"],
                    help="rendered depth maps: drop (mask) or keep the pixels whose nearest face looks away from the camera")
    ap.add_argument("--max_rel_diff", type=float, default=None, metavar="R",
                    help="rendered depth maps: also drop a pixel where depth_est exists and differs by more than R times the "
                         "rendered depth")
    ap.add_argument("--export_blended", default=None, metavar="DIR",
                    help="also write DIR/<scan>/{blended_images,cams,rendered_depth_maps}: the tree fit --dataset blended reads")
    ap.add_argument("--save_image", action="store_true", help="also write depth_mesh/%%08d.jpg, the colour render")


def main(argv=None) -> Dict[str, Dict[str, object]]:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--testpath", required=True, help="the scenes: <testpath>/<scan>/{pair.txt,cams}")
    ap.add_argument("--outdir", required=True, help="the infer output folder: <outdir>/<scan>/{depth_est,cams,images}")
    ap.add_argument("--testlist", required=True, help="text file with one scan name per line")
    ap.add_argument("--mesh", default=None, help="the mesh file; {scan} is replaced (default <outdir>/{scan}_mesh.ply)")
    ap.add_argument("--device", default="cuda")
    add_render_args(ap)
    args = ap.parse_args(argv)
    if args.max_rel_diff is not None and not args.max_rel_diff >= 0:
        ap.error(f"--max_rel_diff must be >= 0, got {args.max_rel_diff}")
    scans = read_testlist(args.testlist)
    out = {}
    for scan in scans:
        ply = (args.mesh or os.path.join(args.outdir, "{scan}_mesh.ply")).format(scan=scan)
        out[scan] = render_scan(os.path.join(args.outdir, scan), ply, os.path.join(args.testpath, scan), back=args.back,
                                max_rel_diff=args.max_rel_diff, save_image=args.save_image, device=args.device)
        if args.export_blended:
            export_blended(scan, args.testpath, args.outdir, args.export_blended)
    return out


if __name__ == "__main__":
    main()
