"""A mesh scored against the photographs of its own scan, on the GPU: PSNR and SSIM of the textured render, with no ground truth
(rules S and C are in include/cds_mvsnet_hip.h).

Every N-th photograph is kept out, the mesh is textured from the rest (``texture.texture_mesh``, unchanged), rendered into the
held-out cameras (``render.render_mesh``, unchanged, then ``cds_photo_shade``: every pixel looked up in its face's atlas cell) and
compared with the photographs under the render's mask (``cds_photo_scores``: squared error per channel, and SSIM over valid-only
11 x 11 Gaussian windows, per channel).  The numbers are a function of the input alone, the same bits run to run.  The hot paths
are the kernels of ``csrc/photo.hip``.  There is no CPU path.

    python -m cds_mvsnet_amd.photo_eval --testpath <scenes> --outdir <out> --testlist <list> [--mesh "<out>/{scan}_mesh.ply"]
        [--holdout N] [--colors texture|vertex] [--back mask|keep] [--texture_scale S] [--texture_max_cell C]
        [--texture_max_size N] [--texture_min_px P] [--texture_level ITER [--texture_level_lambda L]] [--save_renders]
        [--json scores.json]

scores ``<out>/<scan>_mesh.ply`` against ``<out>/<scan>/images/%08d.jpg`` with the cameras of ``<out>/<scan>/cams`` for the views
of ``<testpath>/<scan>/pair.txt``, prints one line per scan and the means over the list.  ``--holdout N`` (N >= 2) keeps the views
at the positions 0, N, 2N, ... of pair.txt out of the texture and scores only them; ``--holdout 0`` textures from all views and
scores all of them: a consistency score, not a held-out one.  ``--colors vertex`` scores the interpolated vertex colours instead of
a texture: the mesh's vertex colours were fused from EVERY view, so no view is truly held out in that mode, whatever --holdout says.
``infer ... --fuse --mesh_voxel SIZE --photo_eval [--photo_holdout N]`` scores the mesh right after it is written.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check
from .mesh import check_mesh_device, check_mesh_layout, load_mesh
from .mvs_io import ScanFolder, read_pair_file, read_testlist
from .render import MAX_CHUNK, camera_table, render_mesh
from .texture import MAX_SIZE, add_texture_args, texture_kwargs, texture_mesh

Tensor = torch.Tensor

WINDOW = 11                    # the side of the SSIM window
TILE = 16                      # CDS_PHOTO_TILE
RECORD = 8                     # CDS_PHOTO_RECORD


def gauss_table() -> List[float]:
    """The window's weights of rule C: exp(-(i - 5)^2 / 4.5), divided by their sum in ascending order."""
    g = [math.exp(-((i - 5) ** 2) / 4.5) for i in range(WINDOW)]
    s = 0.0
    for v in g:
        s += v
    return [v / s for v in g]


def _on(dev, what: str, **tensors) -> None:
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a tensor, got {type(t)}")
        if not t.is_cuda or (dev is not None and t.device != dev):
            raise RuntimeError(f"{what}: {name} must be on {dev if dev is not None else 'a ROCm device'}; there is no CPU fallback")


# ------------------------------------------------------------------------------------------------------------------- rule S
def shade_views(mesh: Dict[str, Tensor], tex: Dict[str, Tensor], cams: Tensor, h: int, w: int, chunk: int = 8) -> Dict[str, Tensor]:
    """``mesh``: vertices float32 [NV,3] and faces int32 [NF,3] on one ROCm device; ``tex``: "uv" int32 [NF,3,2] and "atlas" uint8
    [H,W,3] on that device, as ``texture.texture_mesh`` returns them or as an OBJ of ``texture.write_textured_obj`` gives them back;
    ``cams`` [V,2,4,4] on any device.  Renders the mesh with ``render.render_mesh`` and shades every pixel from the atlas cell of
    its face (rule S) -> {"image" uint8 [V,h,w,3], "face" int32, "valid" uint8, "depth" float32 [V,h,w]}.  A pixel without a
    face, and one whose face has no cell inside the atlas, is black.  ``chunk`` views go into one launch; the result does not
    depend on it."""
    what = "shade_views"
    vert, faces = mesh["vertices"], mesh["faces"]
    nv, nf = check_mesh_layout(vert, None, faces, what), int(faces.shape[0])
    uv, atlas = tex["uv"], tex["atlas"]
    if not isinstance(uv, torch.Tensor) or uv.dtype != torch.int32 or tuple(uv.shape) != (nf, 3, 2):
        raise ValueError(f"{what}: uv must be an int32 [{nf},3,2] tensor, got {getattr(uv, 'dtype', type(uv))} {tuple(getattr(uv, 'shape', ()))}")
    if not isinstance(atlas, torch.Tensor) or atlas.dtype != torch.uint8 or atlas.dim() != 3 or atlas.shape[2] != 3:
        raise ValueError(f"{what}: the atlas must be a uint8 [H,W,3] tensor, got {getattr(atlas, 'dtype', type(atlas))} "
                         f"{tuple(getattr(atlas, 'shape', ()))}")
    ah, aw = int(atlas.shape[0]), int(atlas.shape[1])
    if (ah, aw) != (0, 0) and not (4 <= aw <= MAX_SIZE and aw & (aw - 1) == 0 and ah in (aw, aw // 2)):
        raise ValueError(f"{what}: an atlas of {aw} x {ah}: the width must be a power of two in 4..{MAX_SIZE}, the height the same or its half")
    chunk = int(chunk)
    if not (1 <= chunk <= MAX_CHUNK):
        raise ValueError(f"{what}: chunk must lie in 1..{MAX_CHUNK}, got {chunk}")
    maps = render_mesh(vert, faces, cams, h, w, chunk=chunk)                # §1.10, unchanged: it checks cams, h, w and the device
    dev = check_mesh_device(vert, None, faces, what)
    _on(dev, what, uv=uv, atlas=atlas)
    h, w, v = int(h), int(w), int(cams.shape[0])
    out = {"image": torch.zeros((v, h, w, 3), dtype=torch.uint8, device=dev), "face": maps["face"], "valid": maps["valid"],
           "depth": maps["depth"]}
    if v == 0:
        return out
    vert, faces, uv, atlas = vert.contiguous(), faces.contiguous(), uv.contiguous(), atlas.contiguous()
    tab = camera_table(cams).to(dev)
    lib, hw = _lib.load(), h * w
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for v0 in range(0, v, chunk):
            n = min(chunk, v - v0)
            check(lib.cds_photo_shade(vert.data_ptr(), nv, faces.data_ptr(), nf, uv.data_ptr(), atlas.data_ptr(), ah, aw,
                                      tab.data_ptr() + 8 * tab.shape[1] * v0, n, out["face"].data_ptr() + 4 * v0 * hw, h, w,
                                      out["image"].data_ptr() + 3 * v0 * hw, stream), "cds_photo_shade")
    return out


# ------------------------------------------------------------------------------------------------------------------- rule C
def image_scores(a: Tensor, b: Tensor, mask: Tensor, ssim_map: bool = False) -> Dict[str, Tensor]:
    """``a``, ``b`` uint8 [V,h,w,3] and ``mask`` uint8 or bool [V,h,w] on one ROCm device (a pixel counts where mask != 0) ->
    per view, on that device: "n_px" int64 [V], "sse" int64 [V,3] (exact), "n_win" int64 [V] (the 11 x 11 windows that lie
    inside the mask), "ssim_sum" float64 [V,3], and from them float64 [V]
    "psnr" = 10 log10(255^2 3 n_px / sum sse) (inf without error, NaN without pixels),
    "ssim" = sum ssim_sum / (3 n_win) (NaN without windows), "coverage" = n_px / (h w).
    ``ssim_map``: also "ssim_map" float64 [V,3,h-10,w-10], NaN where a window does not count ([V,3,0,0] for h or w < 11)."""
    what = "image_scores"
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
            raise ValueError(f"{what}: {name} must be a uint8 [V,h,w,3] tensor, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    v, h, w = (int(x) for x in a.shape[:3])
    if tuple(b.shape) != tuple(a.shape):
        raise ValueError(f"{what}: a is {tuple(a.shape)} and b {tuple(b.shape)}")
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool) or tuple(mask.shape) != (v, h, w):
        raise ValueError(f"{what}: mask must be a uint8 or bool [{v},{h},{w}] tensor, got {getattr(mask, 'dtype', type(mask))} "
                         f"{tuple(getattr(mask, 'shape', ()))}")
    if h < 1 or w < 1 or h * w >= 2 ** 31:
        raise ValueError(f"{what}: images of {h} x {w}")
    _on(None, what, a=a)
    dev = a.device
    _on(dev, what, b=b, mask=mask)
    a, b, mask = a.contiguous(), b.contiguous(), mask.to(torch.uint8).contiguous()
    counts = torch.zeros((v, 5), dtype=torch.int64, device=dev)
    sums = torch.zeros((v, 3), dtype=torch.float64, device=dev)
    mh, mw = (h - WINDOW + 1, w - WINDOW + 1) if h >= WINDOW and w >= WINDOW else (0, 0)
    smap = torch.full((v, 3, mh, mw), math.nan, dtype=torch.float64, device=dev) if ssim_map else None
    if v > 0:
        g = (ctypes.c_double * WINDOW)(*gauss_table())
        tiles = ((h + TILE - 1) // TILE) * ((w + TILE - 1) // TILE)
        lib, hw = _lib.load(), h * w
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            ws = torch.empty(min(v, MAX_CHUNK) * tiles * RECORD, dtype=torch.int64, device=dev)
            for v0 in range(0, v, MAX_CHUNK):
                n = min(MAX_CHUNK, v - v0)
                check(lib.cds_photo_scores(a.data_ptr() + 3 * v0 * hw, b.data_ptr() + 3 * v0 * hw, mask.data_ptr() + v0 * hw, g, n, h, w,
                                           ws.data_ptr(), int(ws.numel()), counts.data_ptr() + 8 * 5 * v0, sums.data_ptr() + 8 * 3 * v0,
                                           smap.data_ptr() + 8 * 3 * mh * mw * v0 if ssim_map and mh else None, stream),
                      "cds_photo_scores")
    out = {"n_px": counts[:, 0], "sse": counts[:, 1:4], "n_win": counts[:, 4], "ssim_sum": sums}
    n, e, nw = out["n_px"].double(), out["sse"].sum(1).double(), out["n_win"].double()
    out["psnr"] = 10.0 * torch.log10((65025.0 * (3.0 * n)) / e)              # x / 0 = inf, 0 / 0 = NaN
    out["ssim"] = ((sums[:, 0] + sums[:, 1]) + sums[:, 2]) / (3.0 * nw)
    out["coverage"] = n / float(h * w)
    if ssim_map:
        out["ssim_map"] = smap
    return out


# -------------------------------------------------------------------------------------------------------------------- scans
def _nanmean(vals: Sequence[float]) -> float:
    kept = [x for x in vals if not math.isnan(x)]
    return float(np.mean(kept)) if kept else math.nan


def score_scan(scan_out_folder: str, mesh_ply, pair_folder: str, holdout: int = 0, colors: str = "texture", back: str = "mask",
               save_renders: bool = False, device: str = "cuda", chunk: int = 8, **texture_kw) -> Dict[str, object]:
    """Score a mesh against the images ``<scan_out_folder>/images/%08d.jpg`` with the cameras of ``<scan_out_folder>/cams`` for the
    views of ``<pair_folder>/pair.txt``, in that order, grouped by image size as ``texture.texture_scan`` groups them.
    ``mesh_ply``: a file of ``mesh.write_mesh_ply``, or the mesh dict of the mesh stage on the device.

    ``holdout = N >= 2``: the views at the positions k of pair.txt with k % N == 0 are the test views; the others texture the mesh
    (``texture.texture_mesh`` with ``texture_kw``: scale, max_cell, max_size, min_px, level, level_lambda); the test views are rendered and scored.
    ``holdout = 0``: every view textures and every view is scored, a consistency score and not a held-out one.
    ``colors="vertex"`` scores the vertex-colour render of the rasteriser instead; the mesh's vertex colours were fused from
    EVERY view, so no view is truly held out in that mode.
    ``back``: the mask is the render's valid map ("mask": the nearest face looks at the camera) or face >= 0 ("keep").
    ``save_renders`` writes ``<scan_out_folder>/render_photo/%08d.png``.
    -> {"views": the scored view ids, "psnr", "ssim", "coverage": one float per scored view, "n_px", "n_win": one int per view,
    "mean": {"psnr", "ssim", "coverage"}, each over the views where it is not NaN, "scored": the number of views, "holdout",
    "colors", "back", "textured_from": the number of views behind the texture}."""
    what = "score_scan"
    holdout = int(holdout)
    if holdout != 0 and holdout < 2:
        raise ValueError(f"{what}: holdout must be 0 or >= 2, got {holdout}")
    if colors not in ("texture", "vertex"):
        raise ValueError(f"{what}: colors must be 'texture' or 'vertex', got {colors!r}")
    if back not in ("mask", "keep"):
        raise ValueError(f"{what}: back must be 'mask' or 'keep', got {back!r}")
    dev = torch.device(device)
    mesh = load_mesh(mesh_ply, dev)
    scan = ScanFolder(scan_out_folder)
    vids = [ref for ref, _ in read_pair_file(os.path.join(pair_folder, "pair.txt"))]
    test = [vid for k, vid in enumerate(vids) if holdout == 0 or k % holdout == 0]
    train = [vid for k, vid in enumerate(vids) if holdout == 0 or k % holdout != 0]

    def load(ids):
        groups = scan.groups(ids, scan.image_size).values()               # views by image size, each in pair.txt order
        return [(list(g), torch.from_numpy(np.stack([scan.image(i) for i in g])).to(dev),
                 torch.from_numpy(np.stack([scan.cam(i) for i in g]))) for g in groups]

    tex = None
    if colors == "texture":
        groups = load(train)
        tex, info = texture_mesh(mesh, [img for _, img, _ in groups], [cam for _, _, cam in groups], chunk=chunk, **texture_kw)
        if info["H"] == 0:
            raise ValueError(f"{what}: {scan_out_folder}: a mesh of {info['faces']} faces and {info['views']} views to texture it "
                             f"from (holdout {holdout} of {len(vids)} views): nothing to score")
        if holdout == 0:
            test_groups = groups
    if colors == "vertex" or holdout != 0:
        test_groups = load(test)
    out: Dict[str, object] = {k: [] for k in ("views", "psnr", "ssim", "coverage", "n_px", "n_win")}
    if save_renders:
        os.makedirs(os.path.join(scan_out_folder, "render_photo"), exist_ok=True)
    for ids, img, cam in test_groups:
        h, w = int(img.shape[1]), int(img.shape[2])
        if tex is not None:
            maps = shade_views(mesh, tex, cam, h, w, chunk=chunk)
        else:
            maps = render_mesh(mesh["vertices"], mesh["faces"], cam, h, w, colors=mesh["colors"], chunk=chunk)
        mask = maps["valid"] != 0 if back == "mask" else maps["face"] >= 0
        s = image_scores(maps["image"], img, mask)
        out["views"] += ids
        for k in ("psnr", "ssim", "coverage", "n_px", "n_win"):
            out[k] += s[k].cpu().tolist()
        if save_renders:
            from PIL import Image
            render = maps["image"].cpu().numpy()
            for k, vid in enumerate(ids):
                Image.fromarray(render[k]).save(os.path.join(scan_out_folder, "render_photo", f"{vid:08d}.png"))
    out["mean"] = {k: _nanmean(out[k]) for k in ("psnr", "ssim", "coverage")}
    out.update(scored=len(out["views"]), holdout=holdout, colors=colors, back=back, textured_from=len(train) if tex is not None else 0)
    print(f"{os.path.basename(os.path.normpath(scan_out_folder))}: {format_scores(out)}", flush=True)
    return out


def format_scores(r: Dict[str, object]) -> str:
    kind = (f"held-out score, every {r['holdout']}th view kept out of the texture" if r["holdout"] and r["colors"] == "texture" else
            "consistency score, every view also textures the mesh" if r["colors"] == "texture" else
            "vertex colours, fused from every view: not a held-out score")
    m = r["mean"]
    return f"psnr {m['psnr']:.3f} dB  ssim {m['ssim']:.4f}  coverage {100.0 * m['coverage']:.2f} %  over {r['scored']} views ({kind})"


# ---------------------------------------------------------------------------------------------------------------------- CLI
def main(argv: Optional[Sequence[str]] = None) -> Dict[str, object]:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--testpath", required=True, help="the scenes: <testpath>/<scan>/pair.txt")
    ap.add_argument("--outdir", required=True, help="the infer output folder: <outdir>/<scan>/{cams,images}")
    ap.add_argument("--testlist", required=True, help="text file with one scan name per line")
    ap.add_argument("--mesh", default=None, help="the mesh file; {scan} is replaced (default <outdir>/{scan}_mesh.ply)")
    ap.add_argument("--holdout", type=int, default=0, metavar="N",
                    help="N >= 2 keeps the views at the positions 0, N, 2N, ... of pair.txt out of the texture and scores only them; "
                         "0 (default) textures from all views and scores all: a consistency score, not a held-out one")
    ap.add_argument("--colors", default="texture", choices=["texture", "vertex"],
                    help="score the textured render, or the interpolated vertex colours: those were fused from EVERY view, so no "
                         "view is truly held out in that mode")
    ap.add_argument("--back", default="mask", choices=["mask", "keep"],
                    help="compare where the nearest face looks at the camera (mask), or wherever a face was hit (keep)")
    ap.add_argument("--save_renders", action="store_true", help="also write <outdir>/<scan>/render_photo/%%08d.png")
    ap.add_argument("--json", help="write the per-scan and mean results here")
    ap.add_argument("--device", default="cuda")
    add_texture_args(ap)
    args = ap.parse_args(argv)
    if args.holdout != 0 and args.holdout < 2:
        ap.error(f"--holdout must be 0 or >= 2, got {args.holdout}")
    kw = texture_kwargs(ap, args)
    per_scan = {}
    for scan in read_testlist(args.testlist):
        ply = (args.mesh or os.path.join(args.outdir, "{scan}_mesh.ply")).format(scan=scan)
        per_scan[scan] = score_scan(os.path.join(args.outdir, scan), ply, os.path.join(args.testpath, scan), holdout=args.holdout,
                                    colors=args.colors, back=args.back, save_renders=args.save_renders, device=args.device, **kw)
    mean = {k: _nanmean([r["mean"][k] for r in per_scan.values()]) for k in ("psnr", "ssim", "coverage")}
    print(f"mean over {len(per_scan)} scans: psnr {mean['psnr']:.3f} dB  ssim {mean['ssim']:.4f}  coverage {100.0 * mean['coverage']:.2f} %")
    out = {"scans": per_scan, "mean": mean,
           "settings": {"holdout": args.holdout, "colors": args.colors, "back": args.back, "texture": kw}}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
