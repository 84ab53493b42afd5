"""Depth-map inference harness (the counterpart of the reference's test.py:153-265 `save_depth`).

    python -m cds_mvsnet_amd.infer --testpath <scenes> --testlist <list.txt> --outdir <out> \
        [--resume ckpt.pth] [--refine] [--num_view 5] [--numdepth 192] [--max_h 512 --max_w 640] [--temperature 0.01]
        [--pipeline gpu [--view_cache_mb 2048]] [--ndepths 48,32,8] [--depth_inter_r 4.0,1.5,0.75]

One process per GPU: with `python -m torch.distributed.run --nproc-per-node N -m cds_mvsnet_amd.infer ...` every rank takes
the reference views `idx % world == rank` (independent depth maps, no collective).  Outputs follow the reference layout:
`<out>/<scan>/depth_est/%08d.pfm`, `confidence/%08d.pfm` (3 channels = stage 1-3 confidences), `cams/%08d_cam.txt`,
`images/%08d.jpg`, ready for the fusion step.  `--fuse` then writes `<out>/<scan>.ply` with the normal fusion (fusion.py) or,
with `--filter_method gipuma`, the gipuma-style one (gipuma.py; `--prob_threshold`, `--disp_threshold`, `--num_consistent`),
or, with `--filter_method dynamic`, the dynamic consistency check (fusion.py; `--conf`, `--dyn_dist_base`, `--dyn_rel_base`,
`--dyn_views`).  `--normals` (`--normal_radius`, `--normal_jump`, `--normal_min_pts`; not for gipuma) adds each point's oriented
normal and `--merge_voxel SIZE` (`--merge_min_points K`) merges the scan to one point per occupied voxel;
`--outlier_nb K` (`--outlier_std R`, `--outlier_max_dist d`) and `--outlier_radius r --outlier_min_nb n` then remove the cloud's
outliers, for every fusion method.
`--mesh_voxel SIZE` (`--mesh_trunc T`, `--mesh_min_weight N`; not for gipuma) also writes `<out>/<scan>_mesh.ply`, a triangle mesh
from the same fusion pass (mesh.py); `--mesh_min_component N` / `--mesh_keep_largest K` drop its small connected
components first and `--mesh_simplify CELL` (`--mesh_simplify_placement quadric|mean`) then merges the vertices
of every cell of that side into one, after `--mesh_fill_holes N` has closed the holes of at most N border edges
 and `--mesh_smooth ITER` (`--mesh_smooth_lambda L`, `--mesh_smooth_mu M`,
`--mesh_smooth_max_move D`) has smoothed it; `--mesh_sample SPACING` also writes `<out>/<scan>_surface.ply`, the surface
of that mesh as a cloud; `--mesh_weight angle|conf|angle_conf` and `--mesh_interp` (`--mesh_interp_jump J`) weigh
the pixels and interpolate the depth in the integration.  With `--mesh_voxel`, `--render_mesh` (`--back`, `--max_rel_diff R`, `--save_image`) renders
that mesh into every view, `<out>/<scan>/depth_mesh/%08d.pfm`, and `--export_blended DIR` writes the tree `fit --dataset blended`
trains from (render.py); `--texture` (`--texture_scale S`, `--texture_max_cell C`, `--texture_max_size N`,
`--texture_min_px P`) textures it from the saved images, `<out>/<scan>_textured.{obj,mtl,png}` (texture.py), with
`--texture_level ITER` (`--texture_level_lambda L`) after levelling the seams between faces coloured from different views (§1.19);
`--photo_eval` (`--photo_holdout N`) scores it against the saved images, PSNR and SSIM of its textured render in the views kept
out of the texture (photo_eval.py).
`--save_stages` also writes the three stages' own depth maps, `<out>/<scan>/depth_stage{1,2,3}/%08d.pfm`, at their resolutions
(what evaluations/precision.py scores stage by stage; `python -m cds_mvsnet_amd.depth_eval --folders ...`).

`--pipeline host` (the default) prepares every sample on the host (mvs_io.EvalScenes) and writes its files before the next forward
starts (mvs_io.save_outputs).  `--pipeline gpu` (eval_data.py) decodes each view once per scan, prepares it on the
GPU, keeps it in a cache of `--view_cache_mb` MiB, packs the outputs on the GPU and writes them on a thread while the next forward
runs.  The files are byte-identical for images that need no resize; an image that is not `max_h x max_w` is resized by the
reference's rule (cv2.resize of the float32 image, INTER_LINEAR, no antialiasing) with `gpu` and by PIL's antialiasing BILINEAR on
the uint8 image with `host`: the two pipelines then feed the network different pixels.
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from . import CDSMVSNet, seeded_init_
from .mvs_io import EvalScenes, read_testlist, save_outputs, write_pfm


class _Opaque:
    """Inert stand-in for a class the checkpoint pickles but this process does not have (the reference's
    ``parse_config.ConfigParser`` rides along in its checkpoints): accepts any construction / state, does nothing."""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        pass

    def __call__(self, *a, **k):
        return _Opaque()


_SAFE_BUILTINS = {"set", "frozenset", "list", "dict", "tuple", "int", "float", "bool", "str", "bytes", "bytearray",
                  "complex", "slice", "range", "object"}


# exact globals a tensor state dict needs; everything else in the pickle stream becomes an inert _Opaque
_SAFE_GLOBALS = {
    ("collections", "OrderedDict"), ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_parameter"),
    ("torch._utils", "_rebuild_tensor"), ("torch", "Size"), ("torch", "device"), ("torch", "dtype"),
    ("torch.serialization", "_get_layout"), ("torch._tensor", "_rebuild_from_type_v2"),
    ("_codecs", "encode"), ("numpy", "dtype"), ("numpy", "ndarray"),
    ("numpy.core.multiarray", "_reconstruct"), ("numpy.core.multiarray", "scalar"),
    ("numpy._core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "scalar"),
}
_SAFE_TORCH_ATTRS = ({n for n in dir(torch) if n.endswith("Storage")}
                     | {n for n in dir(torch) if isinstance(getattr(torch, n, None), torch.dtype)})


class _placeholder_pickle:
    """A ``pickle_module`` for ``torch.load`` whose unpickler resolves ONLY an allowlist of globals (the tensor / storage
    rebuild helpers, ``torch.Size`` / ``dtype`` / ``device``, ``OrderedDict``, numpy array reconstruction, a few builtin
    containers) and replaces every other global by :class:`_Opaque` instead of importing it: ``torch.hub.load``,
    ``torch.jit.load`` and the like are NOT resolvable through it -- nor is ``torch.storage._load_from_bytes``, which is a plain
    ``torch.load(..., weights_only=False)`` with the default pickle module in disguise (zip-format state dicts never reference it)."""
    import pickle as _pickle
    __name__ = "cds_mvsnet_amd.infer._placeholder_pickle"

    class Unpickler(_pickle.Unpickler):
        def find_class(self, module, name):
            if (module, name) in _SAFE_GLOBALS or (module == "torch" and name in _SAFE_TORCH_ATTRS) \
                    or (module == "torch.storage" and name in ("TypedStorage", "UntypedStorage")) \
                    or (module == "builtins" and name in _SAFE_BUILTINS):
                return super().find_class(module, name)
            return _Opaque

    @staticmethod
    def load(f, **kw):
        return _placeholder_pickle.Unpickler(f, **kw).load()


def load_checkpoint(model: torch.nn.Module, path: str, trust_pickle: bool = False) -> None:
    """Reference checkpoints: {'state_dict': ...} with a 'module.' prefix when saved under DataParallel (test.py:180-187).

    Loaded with ``weights_only=True`` (tensors only).  The checkpoints the reference ships also pickle their
    ``ConfigParser``, which that mode refuses: pass ``trust_pickle=True`` (``--trust-checkpoint``) to read such a file
    through a restricted unpickler that turns every non-torch class into an inert placeholder (the reference itself
    does a full ``torch.load``).  Keys are checked: anything missing from the file, or unexpected in it, raises (the
    reference loads with ``strict=False`` and silently keeps random weights); exempt are ``num_batches_tracked`` counters and,
    for a model built with ``refine=False``, the ``refine_network.*`` entries of a checkpoint trained with refinement."""
    import pickle
    try:
        ck = torch.load(path, map_location="cpu", weights_only=True)
    except (pickle.UnpicklingError, RuntimeError) as e:          # refused global / legacy format; I/O errors propagate
        if isinstance(e, RuntimeError) and "eights only" not in str(e) and "nsupported" not in str(e):
            raise
        if not trust_pickle:
            raise RuntimeError(f"{path}: not loadable with weights_only=True ({type(e).__name__}: {str(e)[:200]}). "
                               "If the file is trusted, retry with trust_pickle=True / --trust-checkpoint.") from e
        ck = torch.load(path, map_location="cpu", weights_only=False, pickle_module=_placeholder_pickle)
    sd = ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck
    sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
    res = model.load_state_dict(sd, strict=False)
    has_refine = hasattr(model, "refine_network")
    missing = [k for k in res.missing_keys if not k.endswith("num_batches_tracked")]
    unexpected = [k for k in res.unexpected_keys
                  if not k.endswith("num_batches_tracked") and (has_refine or not k.startswith("refine_network."))]
    if missing or unexpected:
        raise RuntimeError(f"{path}: state dict does not match the model: {len(missing)} missing "
                           f"(e.g. {missing[:3]}), {len(unexpected)} unexpected (e.g. {unexpected[:3]})")


def _triple(kind):
    """argparse ``type=`` for one value per stage, "a,b,c" -> (a, b, c): a malformed value is a usage error at parse time."""
    def parse(text: str) -> tuple:
        try:
            vals = tuple(kind(x) for x in str(text).split(","))
        except ValueError:
            vals = ()
        if len(vals) != 3:
            raise argparse.ArgumentTypeError(f"expected three comma-separated {kind.__name__} values (one per stage), got {text!r}")
        return vals
    return parse


def build_model(args) -> torch.nn.Module:
    """The model the flags describe, on the host: --refine, --ndepths, --depth_inter_r, then --resume or seeded synthetic weights."""
    model = CDSMVSNet(refine=args.refine, ndepths=args.ndepths, depth_interals_ratio=args.depth_inter_r)
    if args.resume:
        load_checkpoint(model, args.resume, trust_pickle=args.trust_checkpoint)
    else:
        seeded_init_(model, 0)  # no checkpoint given: deterministic synthetic weights (plumbing runs)
    return model


def _run_host_pipeline(args, model, data, dev, rank, world, last) -> list:
    """--pipeline host: one sample at a time, prepared on the host, its files written before the next forward starts."""
    times = []
    with torch.no_grad():
        for idx in range(rank, len(data), world):
            s = data[idx]
            t0 = time.time()
            imgs = torch.from_numpy(s["imgs"]).unsqueeze(0).to(dev)
            # cameras and the depth range stay on the host: the model needs them there (12 floats per view become kernel
            # arguments), so no device round trip
            cams = {k: torch.from_numpy(v).unsqueeze(0) for k, v in s["proj_matrices"].items()}
            dv = torch.from_numpy(s["depth_values"]).unsqueeze(0)
            out = model(imgs, cams, dv, temperature=args.temperature)
            torch.cuda.synchronize()
            times.append(time.time() - t0)
            confs = [out["stage1"]["photometric_confidence"][0].cpu().numpy(),
                     out["stage2"]["photometric_confidence"][0].cpu().numpy(),
                     out["photometric_confidence"][0].cpu().numpy()]
            save_outputs(args.outdir, s["filename"], out["refined_depth"][0].cpu().numpy(), confs,
                         s["proj_matrices"][last][0], s["imgs"][0])
            if args.save_stages:
                for k in (1, 2, 3):
                    p = os.path.join(args.outdir, s["filename"].format(f"depth_stage{k}", ".pfm"))
                    os.makedirs(os.path.dirname(p), exist_ok=True)
                    write_pfm(p, out[f"stage{k}"]["depth"][0].float().cpu().numpy())
            print(f"[{rank}] {idx + 1}/{len(data)} {s['filename'].format('depth_est', '.pfm')} {times[-1] * 1e3:.1f} ms", flush=True)
    return times


def _run_gpu_pipeline(args, model, scans, scene_args, dev, rank, world, last) -> list:
    """--pipeline gpu: EvalViews -> model -> OutputWriter.  Nothing here waits for the device between two forwards; the writer is
    closed - every byte on disk - before this returns, because the barrier and the fusions that follow read the files back.  The
    time printed per depth map is host wall time from one sample to the next (the device runs behind it); the average is over the
    whole loop, after a final synchronisation."""
    from .eval_data import EvalViews, OutputWriter
    data = EvalViews(args.testpath, scans, device=dev, cache_mb=args.view_cache_mb, rank=rank, world=world, **scene_args)
    n = len(data)
    done = 0
    torch.cuda.synchronize()
    t_start = t0 = time.time()
    with torch.no_grad(), data, OutputWriter(args.outdir) as writer:
        for s in data:
            cams = {k: torch.from_numpy(v).unsqueeze(0) for k, v in s["proj_matrices"].items()}
            dv = torch.from_numpy(s["depth_values"]).unsqueeze(0)
            out = model(s["imgs"], cams, dv, temperature=args.temperature)
            writer.submit(s["filename"], out, s["proj_matrices"][last][0], s["imgs"][0, 0], save_stages=args.save_stages)
            done += 1
            t1 = time.time()
            print(f"[{rank}] {data.order[done - 1] + 1}/{len(data.scenes)} {s['filename'].format('depth_est', '.pfm')} "
                  f"{(t1 - t0) * 1e3:.1f} ms", flush=True)
            t0 = t1
        torch.cuda.synchronize()
    total = time.time() - t_start                             # the writer is closed: the files are on disk
    print(f"[{rank}] view cache: {data.stats['decodes']} decodes, {data.stats['hits']} hits, {data.stats['evictions']} evictions "
          f"over {n} depth maps", flush=True)
    return [total / n] * n if n else []


def run(args) -> float:
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    scans = read_testlist(args.testlist)
    scene_args = dict(nviews=args.num_view, ndepths=args.numdepth, interval_scale=args.interval_scale, max_h=args.max_h,
                      max_w=args.max_w, refine=args.refine, dataset=args.dataset)
    model = build_model(args).to(dev).eval()
    last = "stage4" if args.refine else "stage3"
    if args.pipeline == "gpu":
        times = _run_gpu_pipeline(args, model, scans, scene_args, dev, rank, world, last)
    else:
        times = _run_host_pipeline(args, model, EvalScenes(args.testpath, scans, **scene_args), dev, rank, world, last)
    avg = float(np.mean(times)) if times else 0.0
    what = "upload + forward" if args.pipeline == "host" else "whole loop, files on disk, per depth map"     # not comparable
    print(f"[{rank}] average time ({what}): {avg:.4f} s over {len(times)} depth maps")
    if args.fuse:
        # step 2 of the reference's test.py (pcd_filter, test.py:386-396): scans are independent -> shard over ranks
        from .fusion import cloud_kwargs, filter_depth, format_admitted, format_cloud, format_outliers
        from .gipuma import filter_scan
        from .mesh import SMOOTH_KEYS, format_mesh, mesh_scan, smooth_args

        def fuse(scan, **kw):
            """The cloud alone, or with --mesh_voxel cloud and mesh from one fusion pass."""
            ply = os.path.join(args.outdir, f"{scan}.ply")
            if args.mesh_voxel is None:
                return filter_depth(os.path.join(args.testpath, scan), os.path.join(args.outdir, scan), ply, **kw)
            info = mesh_scan(os.path.join(args.testpath, scan), os.path.join(args.outdir, scan),
                             os.path.join(args.outdir, f"{scan}_mesh.ply"), args.mesh_voxel, args.mesh_trunc, args.mesh_min_weight,
                             cloud_ply=ply, min_component=args.mesh_min_component, keep_largest=args.mesh_keep_largest,
                             simplify=args.mesh_simplify or 0.0, placement=args.mesh_simplify_placement,
                             sample=args.mesh_sample or 0.0, surface_ply=os.path.join(args.outdir, f"{scan}_surface.ply"),
                             weight=args.mesh_weight, interp=args.mesh_interp, interp_jump=args.mesh_interp_jump,
                             **dict(zip(SMOOTH_KEYS, smooth_args(args))), fill_holes=args.mesh_fill_holes or 0, **kw)
            print(f"[{rank}] {scan}_mesh.ply: {format_mesh(info)}", flush=True)
            if args.render_mesh:
                # the mesh just written, from the device tensors, into every view of the scan
                from .render import export_blended, render_scan
                render_scan(os.path.join(args.outdir, scan), info["mesh"], os.path.join(args.testpath, scan), back=args.back,
                            max_rel_diff=args.max_rel_diff, save_image=args.save_image, device=kw.get("device", "cuda"))
                if args.export_blended:
                    export_blended(scan, args.testpath, args.outdir, args.export_blended)
            if args.texture:
                # the mesh just written, from the device tensors, textured from the saved images of the scan
                from .texture import texture_scan
                texture_scan(os.path.join(args.outdir, scan), info["mesh"], os.path.join(args.testpath, scan),
                             os.path.join(args.outdir, f"{scan}_textured"), device=kw.get("device", "cuda"), **args.texture_kw)
            if args.photo_eval:
                # the mesh just written, from the device tensors, scored against the saved images of the scan
                from .photo_eval import score_scan
                score_scan(os.path.join(args.outdir, scan), info["mesh"], os.path.join(args.testpath, scan),
                           holdout=args.photo_holdout or 0, device=kw.get("device", "cuda"), **args.texture_kw)
            return info["cloud"]

        if world > 1:  # every rank's depth maps must be on disk before any scan is fused
            if not torch.distributed.is_initialized():
                torch.distributed.init_process_group("nccl", device_id=dev)
            torch.distributed.barrier()
        for i, scan in enumerate(scans):
            if i % world != rank:
                continue
            if args.filter_method == "gipuma":
                # the reference's gipuma_filter (test.py:419-426) without fusibile: cds_mvsnet_amd.gipuma
                info = filter_scan(os.path.join(args.outdir, scan), os.path.join(args.outdir, f"{scan}.ply"),
                                   prob_threshold=[float(p) for p in args.prob_threshold.split(",")],
                                   disp_threshold=args.disp_threshold, num_consistent=args.num_consistent, device=str(dev),
                                   merge_voxel=args.merge_voxel, merge_min_points=args.merge_min_points, **args.outliers)
                print(f"[{rank}] {scan}.ply: {info['points']} points from {info['views']} views{format_cloud(info)}"
                      f"{format_outliers(info)} (gipuma)",
                      flush=True)
                continue
            if args.filter_method == "dynamic":
                # the dynamic consistency check: one setting for every scene, thresholds graded by view count
                info = fuse(scan, conf=[float(c) for c in args.conf.split(",")], device=str(dev), method="dynamic",
                            dist_base=args.dyn_dist_base, rel_base=args.dyn_rel_base,
                            n_views=[int(v) for v in args.dyn_views.split(",")], **cloud_kwargs(args), **args.outliers)
                print(f"[{rank}] {scan}.ply: {info['points']} points, final mask {info['mean_final_mask']:.3f}, admitted at "
                      f"{format_admitted(info['admitted_at'])}{format_cloud(info)}{format_outliers(info)} (dynamic)", flush=True)
                continue
            info = fuse(scan, conf=[float(c) for c in args.conf.split(",")], thres_disp=args.thres_disp,
                        thres_view=args.thres_view, device=str(dev), **cloud_kwargs(args), **args.outliers)
            print(f"[{rank}] {scan}.ply: {info['points']} points, final mask {info['mean_final_mask']:.3f}{format_cloud(info)}"
                  f"{format_outliers(info)}", flush=True)
    return avg


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--testpath", required=True)
    ap.add_argument("--testlist", required=True)
    ap.add_argument("--outdir", required=True)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--trust-checkpoint", dest="trust_checkpoint", action="store_true",
                    help="allow full unpickling of --resume (the reference's shipped checkpoints need it; runs arbitrary code)")
    ap.add_argument("--refine", action="store_true")
    ap.add_argument("--num_view", type=int, default=5)
    ap.add_argument("--numdepth", type=int, default=192)
    ap.add_argument("--interval_scale", type=float, default=1.06)
    ap.add_argument("--max_h", type=int, default=512)
    ap.add_argument("--max_w", type=int, default=640)
    ap.add_argument("--temperature", type=float, default=0.01)
    ap.add_argument("--dataset", default="dtu", choices=["dtu", "tt", "general"])
    ap.add_argument("--pipeline", default="host", choices=["host", "gpu"],
                    help="host: samples prepared and files written on the host, one depth map at a time (PIL antialiasing BILINEAR when "
                         "an image needs resizing).  gpu: views decoded once per scan, prepared and cached on the GPU, outputs packed on "
                         "the GPU and written on a thread; an image that needs resizing follows the reference's cv2.resize "
                         "INTER_LINEAR rule instead, so the two pipelines DIFFER for such images and agree byte for byte otherwise")
    ap.add_argument("--view_cache_mb", type=float, default=2048.0,
                    help="--pipeline gpu: device memory for prepared views, in MiB (one view is 12 * max_h * max_w bytes)")
    ap.add_argument("--ndepths", type=_triple(int), default=(48, 32, 8), metavar="a,b,c",
                    help="depth hypotheses per stage (the reference's --ndepths; default 48,32,8)")
    ap.add_argument("--depth_inter_r", type=_triple(float), default=(4.0, 1.5, 0.75), metavar="a,b,c",
                    help="depth interval ratio per stage (the reference's --depth_inter_r; default 4.0,1.5,0.75)")
    ap.add_argument("--save_stages", action="store_true",
                    help="also write depth_stage{1,2,3}/%%08d.pfm: the depth map of each stage at its own resolution")
    ap.add_argument("--fuse", action="store_true", help="filter + fuse the saved depth maps into <outdir>/<scan>.ply")
    ap.add_argument("--conf", default="0.0,0.0,0.0", help="per-stage confidence thresholds (test.py:61)")
    ap.add_argument("--thres_view", type=int, default=3)
    ap.add_argument("--thres_disp", type=float, default=1.0)
    ap.add_argument("--filter_method", default="normal", choices=["normal", "gipuma", "dynamic"],
                    help="--fuse with the normal fusion (fusion.py), the gipuma-style one (gipuma.py) or the dynamic "
                         "consistency check (fusion.py, DESIGN §1.7; uses --conf)")
    ap.add_argument("--prob_threshold", default="0.0,0.0,0.0", help="gipuma: per-stage confidence thresholds (test.py:68)")
    ap.add_argument("--disp_threshold", type=float, default=0.2, help="gipuma: disparity threshold (test.py:69)")
    ap.add_argument("--num_consistent", type=int, default=3, help="gipuma: consistent views a point needs (test.py:70)")
    ap.add_argument("--dyn_dist_base", type=float, default=0.25, help="dynamic: re-projection distance per level, in pixels")
    ap.add_argument("--dyn_rel_base", type=float, default=1.0 / 1300.0, help="dynamic: relative depth difference per level")
    ap.add_argument("--dyn_views", default="2,10", metavar="n_min,n_max",
                    help="dynamic: a pixel is kept when n views agree at level n for some n in this range")
    from .fusion import add_cloud_args, add_outlier_args, outlier_kwargs
    add_cloud_args(ap)
    add_outlier_args(ap)
    from .mesh import add_mesh_args, check_clean_args, check_voxel, check_weight_args
    add_mesh_args(ap)
    from .render import add_render_args
    ap.add_argument("--render_mesh", action="store_true",
                    help="--mesh_voxel: render the mesh into every view and write <outdir>/<scan>/depth_mesh/%%08d.pfm (render.py, "
                         "DESIGN §1.10)")
    add_render_args(ap)
    from .texture import add_texture_args, texture_kwargs
    ap.add_argument("--texture", action="store_true",
                    help="--mesh_voxel: texture the mesh from the saved images and write <outdir>/<scan>_textured.{obj,mtl,png} "
                         "(texture.py, DESIGN §1.17)")
    add_texture_args(ap)
    ap.add_argument("--photo_eval", action="store_true",
                    help="--mesh_voxel: score the mesh against the saved images, PSNR and SSIM of its textured render "
                         "(photo_eval.py, DESIGN §1.18); the --texture_* options apply")
    ap.add_argument("--photo_holdout", type=int, default=None, metavar="N",
                    help="--photo_eval: keep the views at the positions 0, N, 2N, ... of pair.txt out of the texture and score only "
                         "them (N >= 2); without it every view textures and is scored, a consistency score")
    args = ap.parse_args(argv)
    args.outliers = outlier_kwargs(args, ap)
    if (args.outlier_nb > 0 or args.outlier_radius > 0) and not args.fuse:
        ap.error("--outlier_nb and --outlier_radius clean the cloud of --fuse: give --fuse as well")
    if args.render_mesh and args.mesh_voxel is None:
        ap.error("--render_mesh renders the mesh of --mesh_voxel: give --fuse --mesh_voxel SIZE as well")
    if not args.render_mesh and (args.export_blended or args.save_image or args.max_rel_diff is not None or args.back != "mask"):
        ap.error("--export_blended, --save_image, --max_rel_diff and --back belong to --render_mesh")
    if args.max_rel_diff is not None and not args.max_rel_diff >= 0:
        ap.error(f"--max_rel_diff must be >= 0, got {args.max_rel_diff}")
    if args.texture and args.mesh_voxel is None:
        ap.error("--texture textures the mesh of --mesh_voxel: give --fuse --mesh_voxel SIZE as well")
    if args.photo_eval and args.mesh_voxel is None:
        ap.error("--photo_eval scores the mesh of --mesh_voxel: give --fuse --mesh_voxel SIZE as well")
    if args.photo_holdout is not None and not args.photo_eval:
        ap.error("--photo_holdout belongs to --photo_eval")
    if args.photo_holdout is not None and args.photo_holdout != 0 and args.photo_holdout < 2:
        ap.error(f"--photo_holdout must be 0 or >= 2, got {args.photo_holdout}")
    args.texture_kw = texture_kwargs(ap, args, args.texture or args.photo_eval)
    check_clean_args(ap, args, args.mesh_voxel is not None)
    args.mesh_interp_jump = check_weight_args(ap, args, args.mesh_voxel is not None)
    if args.mesh_voxel is not None:
        if args.filter_method == "gipuma":
            ap.error("--mesh_voxel is not implemented for --filter_method gipuma (its fused point has no single depth map); "
                     "use normal or dynamic")
        try:
            check_voxel(args.mesh_voxel, args.mesh_trunc, "--mesh_voxel")
        except ValueError as e:
            ap.error(str(e))
    if args.normals and args.filter_method == "gipuma":
        ap.error("--normals is not implemented for --filter_method gipuma (its fused point is an average over views); "
                 "use normal or dynamic")
    return args


def main(argv=None):
    run(parse_args(argv))


if __name__ == "__main__":
    main()
