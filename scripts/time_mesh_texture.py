"""Time the texturing of csrc/mesh_texture.hip on a DTU-shaped scan: the mesh of scripts/time_mesh_simplify.py, simplified.

    python scripts/time_mesh_texture.py [--views 49 --h 864 --w 1152 --voxel 0.35] [--pieces 4000] [--cells 2,4,8] [--scale 1]
        [--rounds 3] [--write profiles/mesh_texture.md]

The scan and its mesh: time_mesh_simplify's (time_tsdf_mesh.render fused and extracted by mesh.TsdfVolume at --voxel, --pieces
tetrahedra put in), simplified by mesh.simplify_mesh (quadric) at each cell of --cells voxels and textured from the scan's own
images and cameras.  texture.texture_mesh is first held to the step-by-step copy below (the same arrays, bit for bit, in both forms
of the votes and of the fill) and then timed.

Reported, each a median with minimum and maximum over --rounds after a warm-up, one process:
  render                    render.render_mesh over all views, 8 per call, without colours (rule 1)
  votes, per pixel / runs   cds_texture_votes over all views with one add per pixel, and with one add per run of equal faces
  best / cells / place      the per-face kernels
  sort and sums             torch between the launches: the stable sort of the sizes, the units, their prefix sums, the one read
  fill, per texel / unit    cds_texture_fill with one thread per texel, and with one thread per 4 x 4 unit
  texture_mesh              the whole call by the host clock around a device synchronise
kernels between HIP events through the C entry points.  With the fill the time its atlas bytes would take to stream at the
6.3 TB/s a streaming kernel reaches on the MI355X, and the ratio.  Recorded values, not thresholds.  There is no CPU fallback:
without a GPU the script fails."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cds_mvsnet_amd import _lib, mesh, render, texture  # noqa: E402
from time_mesh_clean import add_debris  # noqa: E402
from time_tsdf_mesh import STREAM_TBS, render as make_scan, stats  # noqa: E402

STEPS = ("render", "votes, per pixel", "votes, runs", "best", "cells", "sort and sums", "place", "fill, per texel", "fill, per unit")
CHUNK = 8


def timed_texture(lib, m, images, cams, tab, scale, max_cell, min_px=1):
    """texture_mesh's steps with an event around each, both forms of votes and fill -> ({step: ms}, out, info)."""
    vert, col, faces = m["vertices"], m["colors"], m["faces"]
    nv, nf, dev = int(vert.shape[0]), int(faces.shape[0]), vert.device
    v, h, w = (int(x) for x in images.shape[:3])
    stream = torch.cuda.current_stream().cuda_stream
    ms = dict.fromkeys(STEPS, 0.0)
    views = torch.tensor([(3 * h * w * k, h, w) for k in range(v)], dtype=torch.int64).to(dev)     # the table of the fill: offset, h, w

    def span(name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms[name] += a.elapsed_time(b)
        return out

    key = torch.zeros(nf, dtype=torch.int64, device=dev)
    votes = torch.empty((CHUNK, nf), dtype=torch.int32, device=dev)
    other = torch.empty((CHUNK, nf), dtype=torch.int32, device=dev)
    for v0 in range(0, v, CHUNK):
        n = min(CHUNK, v - v0)
        maps = span("render", lambda: render.render_mesh(vert, faces, cams[v0:v0 + n], h, w, chunk=CHUNK))
        votes.zero_()
        other.zero_()
        args = (maps["face"].data_ptr(), maps["valid"].data_ptr(), n, h, w, nf)
        span("votes, per pixel", lambda: _lib.check(lib.cds_texture_votes(*args, other.data_ptr(), 0, stream), "votes"))
        span("votes, runs", lambda: _lib.check(lib.cds_texture_votes(*args, votes.data_ptr(), 1, stream), "votes"))
        if not torch.equal(votes[:n], other[:n]):
            raise SystemExit("the two forms of cds_texture_votes differ")
        span("best", lambda: _lib.check(lib.cds_texture_best(votes.data_ptr(), nf, n, v0, key.data_ptr(), stream), "best"))
        del maps
    view = torch.empty(nf, dtype=torch.int32, device=dev)
    cell = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    uv = torch.empty((nf, 3, 2), dtype=torch.int32, device=dev)
    span("cells", lambda: _lib.check(lib.cds_texture_cells(vert.data_ptr(), nv, faces.data_ptr(), nf, tab.data_ptr(), v, key.data_ptr(),
                                                           min_px, scale, max_cell, view.data_ptr(), cell.data_ptr(), stream), "cells"))

    def sort_and_sums():
        c = cell[:, 2].to(torch.int64)
        order = torch.sort(-c, stable=True).indices
        units = (c[order] >> 2) ** 2
        ends = torch.cumsum(units, 0)
        total, unseen = (int(x) for x in torch.stack([ends[-1], (view < 0).sum()]).cpu())
        return order, ends - units, total, unseen
    order, starts, total, unseen = span("sort and sums", sort_and_sums)
    ah, aw = texture.atlas_size(total)
    span("place", lambda: _lib.check(lib.cds_texture_place(order.data_ptr(), starts.data_ptr(), nf, total, max_cell, cell.data_ptr(),
                                                           uv.data_ptr(), stream), "place"))
    atlas = [torch.empty((ah, aw, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    for per_unit, name in ((0, "fill, per texel"), (1, "fill, per unit")):
        span(name, lambda: _lib.check(lib.cds_texture_fill(vert.data_ptr(), col.data_ptr(), nv, faces.data_ptr(), nf, tab.data_ptr(),
                                                           images.data_ptr(), int(images.numel()), views.data_ptr(), v, view.data_ptr(),
                                                           cell.data_ptr(), order.data_ptr(), starts.data_ptr(), total, max_cell, ah, aw,
                                                           atlas[per_unit].data_ptr(), per_unit, stream), "fill"))
    if not torch.equal(atlas[0], atlas[1]):
        raise SystemExit("the two forms of cds_texture_fill differ")
    info = {"H": ah, "W": aw, "faces": nf, "unseen": unseen, "units": (total, (ah // 4) * (aw // 4)), "views": v}
    return ms, {"atlas": atlas[0], "uv": uv, "view": view, "cell": cell}, info


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
        raise SystemExit("time_mesh_texture.py needs the GPU: nothing is measured without one")
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
    lines = []
    summary = ["| cell, voxels | faces | atlas W x H | units used | unseen faces | cells by size | render ms | kernels and torch ms | "
               "texture_mesh ms |\n|---|---|---|---|---|---|---|---|---|"]
    for cv in (float(x) for x in args.cells.split(",")):
        sm, _ = mesh.simplify_mesh(m, cv * args.voxel, "quadric")
        got, info = texture.texture_mesh(sm, images, cams, scale=args.scale, max_cell=args.max_cell, chunk=CHUNK)     # the check, the warm-up
        _, out, info2 = timed_texture(lib, sm, images, cams, tab, args.scale, args.max_cell)
        for k in ("atlas", "uv", "view", "cell"):
            if not torch.equal(got[k], out[k]):
                raise SystemExit(f"the step-by-step copy differs from texture_mesh in {k} (cell {cv})")
        if info != info2:
            raise SystemExit(f"the step-by-step copy differs from texture_mesh in info: {info} against {info2}")
        sizes, counts = torch.unique(got["cell"][:, 2], return_counts=True)
        by_size = ", ".join(f"{int(s)}: {int(n)}" for s, n in zip(sizes.cpu(), counts.cpu()))
        del got, out
        t = {k: [] for k in STEPS + ("texture_mesh",)}
        for _ in range(args.rounds):
            ms, out, _ = timed_texture(lib, sm, images, cams, tab, args.scale, args.max_cell)
            del out
            for k in STEPS:
                t[k].append(ms[k])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            texture.texture_mesh(sm, images, cams, scale=args.scale, max_cell=args.max_cell, chunk=CHUNK)
            torch.cuda.synchronize()
            t["texture_mesh"].append((time.perf_counter() - t0) * 1e3)
        nf, atlas_bytes = info["faces"], 3 * info["H"] * info["W"]
        floor = atlas_bytes / (STREAM_TBS * 1e12) * 1e3
        med = {k: float(np.median(t[k])) for k in t}
        chosen = med["votes, runs" if texture.VOTE_RUNS else "votes, per pixel"] + med["best"] + med["cells"] + med["sort and sums"] + \
            med["place"] + med["fill, per unit" if texture.FILL_PER_UNIT else "fill, per texel"]
        used, room = info["units"]
        summary.append(f"| {cv:g} | {nf} | {info['W']} x {info['H']} | {100.0 * used / room:.1f} % | {100.0 * info['unseen'] / nf:.2f} % | "
                       f"{by_size} | {med['render']:.2f} | {chosen:.2f} | {med['texture_mesh']:.2f} |")
        lines += [f"### Simplified at {cv:g} voxels: {nf} faces\n", f"{info}\n", "| step | median ms | min | max |\n|---|---|---|---|"]
        lines += [f"| {k} | {stats(t[k])} |" for k in STEPS]
        lines.append(f"| texture_mesh, host clock | {stats(t['texture_mesh'])} |\n")
        lines.append(f"The atlas is {atlas_bytes / 1e6:.1f} MB: {floor:.4f} ms to stream at {STREAM_TBS} TB/s.  fill per texel takes "
                     f"{med['fill, per texel'] / floor:.1f} times that, fill per unit {med['fill, per unit'] / floor:.1f} times.\n")
        print("\n".join(lines[-(len(STEPS) + 6):]), flush=True)
        del sm
        torch.cuda.empty_cache()
    print("\n".join(summary), flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Texturing a scan's mesh on the MI355X (`csrc/mesh_texture.hip`)\n\n"
                    f"`python scripts/time_mesh_texture.py --views {args.views} --h {args.h} --w {args.w} --voxel {args.voxel} --pieces "
                    f"{args.pieces} --cells {args.cells} --scale {args.scale:g} --rounds {args.rounds}`: {args.rounds} repetitions after a "
                    "warm-up, one process, one MI355X.  Steps between HIP events with a synchronise after each, texture_mesh by the host "
                    "clock around a device synchronise.  No threshold: nothing before this does the step.  Recorded values.  "
                    "`kernels and torch` sums the forms texture_mesh uses "
                    f"(votes {'by runs' if texture.VOTE_RUNS else 'per pixel'}, fill {'per unit' if texture.FILL_PER_UNIT else 'per texel'}).\n\n"
                    + "\n".join(summary) + "\n\n" + "\n".join(lines) + "\n")
        print(f"wrote {args.write}", flush=True)


if __name__ == "__main__":
    main()
