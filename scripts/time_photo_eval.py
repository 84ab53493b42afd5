"""Time the photometric score of csrc/photo.hip on a DTU-shaped scan: the mesh of scripts/time_mesh_simplify.py, simplified.

    python scripts/time_photo_eval.py [--views 49 --h 864 --w 1152 --voxel 0.35] [--pieces 4000] [--cells 2,4,8] [--scale 1]
        [--rounds 3] [--write profiles/photo_eval.md]

The scan and its mesh: time_mesh_texture's (time_tsdf_mesh.render fused and extracted by mesh.TsdfVolume at --voxel, --pieces
tetrahedra put in), simplified by mesh.simplify_mesh (quadric) at each cell of --cells voxels, textured from the scan's own images
and cameras (texture.texture_mesh), then rendered into every view and compared with the images.  photo_eval.shade_views and
photo_eval.image_scores are first held to the step-by-step copy below (the same arrays, bit for bit) and then timed.

Reported, each a median with minimum and maximum over --rounds after a warm-up, one process:
  render        render.render_mesh over all views, 8 per call, without colours
  shade         cds_photo_shade over all views, 8 per call
  scores        cds_photo_scores over all views, 32 per call, without the map
  shade_views   the whole call by the host clock around a device synchronise
  image_scores  likewise
kernels between HIP events through the C entry points.  With shade the time its own bytes would take to stream at the 6.3 TB/s a
streaming kernel reaches on the MI355X (the face map in, the image out: 7 B per pixel; the atlas once), with scores likewise
(both images and the mask in: 7 B per pixel; the tile records out), and the fraction of that rate reached.  Recorded values, not
thresholds.  There is no CPU fallback: without a GPU the script fails."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cds_mvsnet_amd import _lib, mesh, photo_eval, render, texture  # noqa: E402
from time_mesh_clean import add_debris  # noqa: E402
from time_tsdf_mesh import STREAM_TBS, render as make_scan, stats  # noqa: E402

STEPS = ("render", "shade", "scores")
CHUNK = 8


def timed_score(lib, m, tex, images, cams, tab):
    """shade_views' and image_scores' steps with an event around each -> ({step: ms}, image, counts, sums)."""
    vert, faces, uv, atlas = m["vertices"], m["faces"], tex["uv"], tex["atlas"]
    nv, nf, dev = int(vert.shape[0]), int(faces.shape[0]), vert.device
    v, h, w = (int(x) for x in images.shape[:3])
    hw = h * w
    stream = torch.cuda.current_stream().cuda_stream
    ms = dict.fromkeys(STEPS, 0.0)

    def span(name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms[name] += a.elapsed_time(b)
        return out

    image = torch.empty((v, h, w, 3), dtype=torch.uint8, device=dev)
    mask = torch.empty((v, h, w), dtype=torch.uint8, device=dev)
    for v0 in range(0, v, CHUNK):
        n = min(CHUNK, v - v0)
        maps = span("render", lambda: render.render_mesh(vert, faces, cams[v0:v0 + n], h, w, chunk=CHUNK))
        span("shade", lambda: _lib.check(lib.cds_photo_shade(vert.data_ptr(), nv, faces.data_ptr(), nf, uv.data_ptr(), atlas.data_ptr(),
                                                            int(atlas.shape[0]), int(atlas.shape[1]),
                                                            tab.data_ptr() + 8 * render.CAM_DOUBLES * v0, n, maps["face"].data_ptr(), h, w,
                                                            image.data_ptr() + 3 * v0 * hw, stream), "shade"))
        mask[v0:v0 + n] = maps["valid"]
        del maps
    g = (ctypes.c_double * photo_eval.WINDOW)(*photo_eval.gauss_table())
    tiles = ((h + photo_eval.TILE - 1) // photo_eval.TILE) * ((w + photo_eval.TILE - 1) // photo_eval.TILE)
    ws = torch.empty(min(v, render.MAX_CHUNK) * tiles * photo_eval.RECORD, dtype=torch.int64, device=dev)
    counts = torch.zeros((v, 5), dtype=torch.int64, device=dev)
    sums = torch.zeros((v, 3), dtype=torch.float64, device=dev)
    for v0 in range(0, v, render.MAX_CHUNK):
        n = min(render.MAX_CHUNK, v - v0)
        span("scores", lambda: _lib.check(lib.cds_photo_scores(image.data_ptr() + 3 * v0 * hw, images.data_ptr() + 3 * v0 * hw,
                                                              mask.data_ptr() + v0 * hw, g, n, h, w, ws.data_ptr(), int(ws.numel()),
                                                              counts.data_ptr() + 40 * v0, sums.data_ptr() + 24 * v0, None, stream),
                                          "scores"))
    return ms, image, mask, counts, sums


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--h", type=int, default=864)
    ap.add_argument("--w", type=int, default=1152)
    ap.add_argument("--voxel", type=float, default=0.35)
    ap.add_argument("--pieces", type=int, default=4000)
    ap.add_argument("--cells", default="2,4,8", help="simplification cell sides in voxels")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--max_cell", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--write", default=None, help="markdown file to record the result in")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_photo_eval.py needs the GPU: nothing is measured without one")
    depths, masks, images, cams, points = make_scan(args.views, args.h, args.w)
    vol = mesh.TsdfVolume(points, args.voxel)
    vol.integrate(depths, masks.to(torch.uint8), images, cams)
    scan = vol.extract(2)
    del vol, points, depths, masks
    m = add_debris(scan, args.pieces)
    del scan
    torch.cuda.empty_cache()
    print(f"mesh: {int(m['vertices'].shape[0])} vertices, {int(m['faces'].shape[0])} faces", flush=True)
    lib = _lib.load()
    tab = render.camera_table(cams).cuda()
    v, h, w = args.views, args.h, args.w
    px = v * h * w
    tiles = ((h + photo_eval.TILE - 1) // photo_eval.TILE) * ((w + photo_eval.TILE - 1) // photo_eval.TILE)
    lines = []
    summary = ["| cell, voxels | faces | atlas W x H | psnr dB | ssim | coverage | render ms | shade ms | of the streaming rate | scores ms | "
               "of the streaming rate | shade_views ms | image_scores ms |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for cv in (float(x) for x in args.cells.split(",")):
        sm, _ = mesh.simplify_mesh(m, cv * args.voxel, "quadric")
        tex, info = texture.texture_mesh(sm, images, cams, scale=args.scale, max_cell=args.max_cell, chunk=CHUNK)
        got = photo_eval.shade_views(sm, tex, cams, h, w, chunk=CHUNK)                                         # the check, the warm-up
        sc = photo_eval.image_scores(got["image"], images, got["valid"])
        _, image, mask, counts, sums = timed_score(lib, sm, tex, images, cams, tab)
        same = torch.equal(got["image"], image) and torch.equal(got["valid"], mask) and torch.equal(sc["ssim_sum"], sums) and \
            torch.equal(torch.cat([sc["n_px"][:, None], sc["sse"], sc["n_win"][:, None]], 1), counts)
        if not same:
            raise SystemExit(f"the step-by-step copy differs from shade_views / image_scores (cell {cv})")
        psnr, ssim, cov = (float(sc[k][~torch.isnan(sc[k])].mean()) for k in ("psnr", "ssim", "coverage"))
        del got, sc, image, mask
        t = {k: [] for k in STEPS + ("shade_views", "image_scores")}
        for _ in range(args.rounds):
            ms, image, mask, _, _ = timed_score(lib, sm, tex, images, cams, tab)
            for k in STEPS:
                t[k].append(ms[k])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            photo_eval.image_scores(image, images, mask)
            torch.cuda.synchronize()
            t["image_scores"].append((time.perf_counter() - t0) * 1e3)
            del image, mask
            t0 = time.perf_counter()
            photo_eval.shade_views(sm, tex, cams, h, w, chunk=CHUNK)
            torch.cuda.synchronize()
            t["shade_views"].append((time.perf_counter() - t0) * 1e3)
        nf, atlas_bytes = info["faces"], 3 * info["H"] * info["W"]
        shade_bytes, score_bytes = 7 * px + atlas_bytes, 7 * px + 8 * photo_eval.RECORD * tiles * v
        floor = {"shade": shade_bytes / (STREAM_TBS * 1e12) * 1e3, "scores": score_bytes / (STREAM_TBS * 1e12) * 1e3}
        med = {k: float(np.median(t[k])) for k in t}
        summary.append(f"| {cv:g} | {nf} | {info['W']} x {info['H']} | {psnr:.2f} | {ssim:.4f} | {100.0 * cov:.1f} % | {med['render']:.2f} | "
                       f"{med['shade']:.3f} | {100.0 * floor['shade'] / med['shade']:.1f} % | {med['scores']:.3f} | "
                       f"{100.0 * floor['scores'] / med['scores']:.1f} % | {med['shade_views']:.2f} | {med['image_scores']:.2f} |")
        lines += [f"### Simplified at {cv:g} voxels: {nf} faces\n", f"{info}\n", "| step | median ms | min | max |\n|---|---|---|---|"]
        lines += [f"| {k} | {stats(t[k])} |" for k in STEPS]
        lines += [f"| shade_views, host clock | {stats(t['shade_views'])} |", f"| image_scores, host clock | {stats(t['image_scores'])} |\n"]
        lines.append(f"shade moves {shade_bytes / 1e6:.1f} MB ({v} face maps, {v} images, the atlas of {atlas_bytes / 1e6:.1f} MB once): "
                     f"{floor['shade']:.4f} ms to stream at {STREAM_TBS} TB/s, {med['shade'] / floor['shade']:.1f} times that measured.  "
                     f"scores moves {score_bytes / 1e6:.1f} MB (7 B per pixel in, {tiles} records of {8 * photo_eval.RECORD} B per view "
                     f"out): {floor['scores']:.4f} ms to stream, {med['scores'] / floor['scores']:.1f} times that measured.\n")
        print("\n".join(lines[-(len(STEPS) + 6):]), flush=True)
        del sm, tex
        torch.cuda.empty_cache()
    print("\n".join(summary), flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Scoring a scan's mesh against its photographs on the MI355X (`csrc/photo.hip`)\n\n"
                    f"`python scripts/time_photo_eval.py --views {args.views} --h {args.h} --w {args.w} --voxel {args.voxel} --pieces "
                    f"{args.pieces} --cells {args.cells} --scale {args.scale:g} --rounds {args.rounds}`: {args.rounds} repetitions after a "
                    "warm-up, one process, one MI355X.  Steps between HIP events with a synchronise after each, shade_views and "
                    "image_scores by the host clock around a device synchronise.  No threshold: nothing before this does the step.  "
                    "Recorded values.  All views texture the mesh and all are scored (the consistency score): psnr, ssim and coverage "
                    "are the means over the views.  `of the streaming rate`: the time the kernel's own bytes would take at "
                    f"{STREAM_TBS} TB/s over the time measured.\n\n" + "\n".join(summary) + "\n\n" + "\n".join(lines) + "\n")
        print(f"wrote {args.write}", flush=True)


if __name__ == "__main__":
    main()
