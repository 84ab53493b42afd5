"""Time the rasteriser of csrc/raster.hip on a DTU-shaped scan: the mesh of scripts/time_tsdf_mesh.py rendered into its views.

    python scripts/time_render_mesh.py [--views 49 --h 864 --w 1152 --voxel 0.35] [--rounds 5] [--write profiles/render_mesh.md]

The scan and its mesh: time_tsdf_mesh.render (the height field of synth.make_fusion_scene from --views cameras), fused and
extracted by mesh.TsdfVolume at --voxel.  The mesh is then rendered into the same views at the same size.

Reported, each a median with minimum and maximum over --rounds after a warm-up of every variant, chunk 1 and chunk 8 alternating
inside every round, one process:
  project / faces / large / resolve   the four launches of render_mesh between HIP events, through the C entry points in
                                      render_mesh's order, summed over the launches of one scan (49 and 7 per kernel)
  list                                render.large_list between faces and large: a reduction over the class bytes and, when one
                                      is set, torch.nonzero (both wait for the device)
  render_mesh                         the whole call by the host clock around a device synchronise
With each kernel the bytes it cannot avoid, computed from the shapes (below), and the fraction of the 6.3 TB/s a streaming kernel
reaches on the MI355X that they are of its time.  Gathers (the snapped corners and camera-space points of a face, 24 + 72 B)
are counted once per use although neighbouring faces share them in cache; the atomics are counted at 8 B per large-list entry
only where stated.  Before anything is timed the outputs of chunk 1 and chunk 8 are compared: they must be torch.equal.
Recorded values, not thresholds.  There is no CPU fallback: without a GPU the script fails."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cds_mvsnet_amd import _lib, mesh, render  # noqa: E402
from time_tsdf_mesh import STREAM_TBS, render as make_scan, stats  # noqa: E402

KERNELS = ("project", "faces", "list", "large", "resolve")


def timed_chunks(lib, m, tab, h, w, chunk, large_px, out):
    """render_mesh's loop with an event between the launches -> {kernel: ms over the scan}, and the counts the byte model needs."""
    v, nv, nf, hw = tab.shape[0], m["vertices"].shape[0], m["faces"].shape[0], h * w
    n = min(chunk, v)
    xy = torch.empty((n, nv, 2), dtype=torch.int32, device="cuda")
    xc = torch.empty((n, nv, 3), dtype=torch.float64, device="cuda")
    keys = torch.empty((n, h, w), dtype=torch.int64, device="cuda")
    large = torch.empty((n, nf), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ms = dict.fromkeys(KERNELS, 0.0)
    n_large = 0
    for v0 in range(0, v, chunk):
        n = min(chunk, v - v0)
        cam = tab.data_ptr() + 8 * render.CAM_DOUBLES * v0
        keys.fill_(-1)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record()
        _lib.check(lib.cds_raster_project(m["vertices"].data_ptr(), nv, cam, n, xy.data_ptr(), xc.data_ptr(), stream), "project")
        ev[1].record()
        _lib.check(lib.cds_raster_faces(m["faces"].data_ptr(), nf, nv, cam, n, xy.data_ptr(), xc.data_ptr(), h, w, large_px,
                                        keys.data_ptr(), large.data_ptr(), stream), "faces")
        ev[2].record()
        todo = render.large_list(large[:n])
        ev[3].record()
        _lib.check(lib.cds_raster_large(todo.data_ptr(), int(todo.numel()), m["faces"].data_ptr(), nf, nv, cam, n, xy.data_ptr(),
                                        xc.data_ptr(), h, w, keys.data_ptr(), stream), "large")
        ev[4].record()
        _lib.check(lib.cds_raster_resolve(keys.data_ptr(), m["faces"].data_ptr(), nf, nv, cam, n, xc.data_ptr(),
                                          m["colors"].data_ptr(), h, w, out["depth"].data_ptr() + 4 * v0 * hw,
                                          out["face"].data_ptr() + 4 * v0 * hw, out["front"].data_ptr() + v0 * hw,
                                          out["valid"].data_ptr() + v0 * hw, out["image"].data_ptr() + 3 * v0 * hw, stream), "resolve")
        ev[5].record()
        torch.cuda.synchronize()
        for k, name in enumerate(KERNELS):
            ms[name] += ev[k].elapsed_time(ev[k + 1])
        n_large += int(todo.numel())
    return ms, n_large


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--h", type=int, default=864)
    ap.add_argument("--w", type=int, default=1152)
    ap.add_argument("--voxel", type=float, default=0.35)
    ap.add_argument("--large_px", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--write", default=None, help="markdown file to record the result in")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_render_mesh.py needs the GPU: nothing is measured without one")
    V, h, w = args.views, args.h, args.w
    depths, masks, images, cams, points = make_scan(V, h, w)
    vol = mesh.TsdfVolume(points, args.voxel)
    vol.integrate(depths, masks.to(torch.uint8), images, cams)
    m = vol.extract(2)
    del vol, points, images
    torch.cuda.empty_cache()
    nv, nf = int(m["vertices"].shape[0]), int(m["faces"].shape[0])
    print(f"mesh: {nv} vertices, {nf} faces", flush=True)

    chunks = (1, 8)
    outs = {c: render.render_mesh(m["vertices"], m["faces"], cams, h, w, colors=m["colors"], chunk=c, large_px=args.large_px)
            for c in chunks}
    for k in outs[1]:
        if not torch.equal(outs[1][k], outs[8][k]):
            raise SystemExit(f"chunk 1 and chunk 8 disagree in {k}")
    out = outs[8]
    del outs
    hit = out["face"] >= 0
    n_hit, n_valid = int(hit.sum()), int(out["valid"].sum())
    both = (depths > 0) & masks & (out["valid"] != 0)
    rel = ((out["depth"] - depths).abs() / depths)[both]
    rel_med, rel_99 = float(rel.median()), float(torch.quantile(rel[:: max(1, rel.numel() // 4000000)], 0.99))

    lib = _lib.load()
    tab = render.camera_table(cams).cuda()
    for c in chunks:                                                   # warm-up of the timed path
        timed_chunks(lib, m, tab, h, w, c, args.large_px, out)
    t = {c: {k: [] for k in KERNELS + ("render_mesh",)} for c in chunks}
    n_large = {}
    for _ in range(args.rounds):
        for c in chunks:
            ms, n_large[c] = timed_chunks(lib, m, tab, h, w, c, args.large_px, out)
            for k in KERNELS:
                t[c][k].append(ms[k])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            render.render_mesh(m["vertices"], m["faces"], cams, h, w, colors=m["colors"], chunk=c, large_px=args.large_px)
            torch.cuda.synchronize()
            t[c]["render_mesh"].append((time.perf_counter() - t0) * 1e3)

    hw = h * w
    nbytes = {"project": V * nv * (12 + 8 + 24),                      # read a vertex, write X, Y and Xc
              "faces": V * nf * (12 + 24 + 1) + V * hw * 8,            # indices, three snapped corners, the class byte; the key fill
              "list": V * nf * 1,                                      # the class bytes read once
              "large": n_large[8] * (8 + 12 + 24 + 72 + 8),            # entry, indices, corners, points, at least one atomic
              "resolve": V * hw * (8 + 13) + n_hit * (12 + 72 + 9)}    # key in, five outputs out; a hit gathers its face

    lines = [f"## One scan: {V} views of {w}x{h}, the mesh of voxel {args.voxel}, large_px {args.large_px}\n",
             f"{nv} vertices and {nf} faces; {100.0 * n_hit / (V * hw):.1f} % of the pixels are hit, {100.0 * n_valid / (V * hw):.1f} % "
             f"valid (front-facing); {n_large[8]} (view, face) pairs of {V * nf} go to the wave path.  Where the scan's own depth map "
             f"and the rendered one both exist they differ by {rel_med:.2e} of the depth in the median and {rel_99:.2e} at the 99th "
             "percentile.  The outputs of 1 and 8 views per launch are equal.\n"]
    for c in chunks:
        launches = (V + c - 1) // c
        lines += [f"### {c} view(s) per launch ({launches} launches of each kernel), ms over the scan\n",
                  "| launch | median ms | min | max | GB it cannot avoid | fraction of 6.3 TB/s |\n|---|---|---|---|---|---|"]
        for k in KERNELS:
            med = float(np.median(t[c][k]))
            floor = nbytes[k] / (STREAM_TBS * 1e12) * 1e3
            lines.append(f"| {k} | {stats(t[c][k])} | {nbytes[k] / 1e9:.2f} | {floor / med if med > 0 else 0.0:.2f} |")
        total = sum(float(np.median(t[c][k])) for k in KERNELS)
        lines.append(f"| sum of the five | {total:.3f} | | | | |")
        lines.append(f"| render_mesh, host clock | {stats(t[c]['render_mesh'])} | | |\n")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Rendering a mesh into the views of a scan on the MI355X (`csrc/raster.hip`)\n\n"
                    f"`python scripts/time_render_mesh.py --views {V} --h {h} --w {w} --voxel {args.voxel} --large_px {args.large_px} "
                    f"--rounds {args.rounds}`: {args.rounds} rounds after a warm-up of every variant, 1 and 8 views per launch "
                    "alternating inside each round, one process, one MI355X.  Kernels between HIP events, render_mesh by the host "
                    "clock around a device synchronise.  Recorded values, not thresholds.\n\n" + text + "\n")
        print(f"wrote {args.write}", flush=True)


if __name__ == "__main__":
    main()
