"""Time the smoothing of csrc/mesh_smooth.hip on a DTU-shaped scan: the mesh of scripts/time_tsdf_mesh.py.

    python scripts/time_mesh_smooth.py [--views 49 --h 864 --w 1152 --voxel 0.35] [--iterations 10] [--cell 2] [--rounds 3]
        [--write profiles/mesh_smooth.md]

The scan and its mesh: time_tsdf_mesh.render fused and extracted by mesh.TsdfVolume at --voxel.  mesh.smooth_mesh is first held to
the step-by-step copy below (the same positions, bit for bit) and then timed.

Reported, each a median with minimum and maximum over --rounds after a warm-up, one process:
  count / offsets / fill / long / finish
                   the steps of the adjacency build between HIP events, kernels through the C entry points: the counting pass,
                   the prefix sum with the search for long segments and the one host read, the fill pass, the torch sort of the
                   segments longer than CDS_MESH_ADJ_SMALL, the finishing kernel
  step             one launch of cds_mesh_smooth_step_f32, over the 2 x --iterations launches of a run
  limit            cds_mesh_smooth_limit_f32
  smooth_mesh      the whole call (adjacency, --iterations iterations, limit, statistics) by the host clock around a synchronise
  simplify_mesh    mesh.simplify_mesh(cell = --cell voxels, quadric) on the same mesh in the same run, by the same clock, for scale
With the step kernel its streaming floor: per vertex its own position (12 B), start and deg (8 B), 4 deg index bytes, 12 B
written, and its neighbours' positions counted ONCE per vertex of the mesh (12 B), as if every gathered row came from cache after
its first use; and the fraction of the 6.3 TB/s a streaming kernel reaches on the MI355X that this is of its time.  Recorded values,
not thresholds.  There is no CPU fallback: without a GPU the script fails."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cds_mvsnet_amd import _lib, mesh  # noqa: E402
from time_tsdf_mesh import STREAM_TBS, render as make_scan, stats  # noqa: E402

BUILD = ("count", "offsets", "fill", "long", "finish")


def timed_smooth(lib, m, iterations, lam, mu):
    """smooth_mesh's steps with an event between them -> ({step: ms}, [ms per step launch], limit ms, positions, adjacency)."""
    vert, faces = m["vertices"], m["faces"]
    nv, nf, dev = vert.shape[0], faces.shape[0], vert.device
    stream = torch.cuda.current_stream().cuda_stream
    ms = dict.fromkeys(BUILD, 0.0)

    def span(name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if name is not None:
            ms[name] += a.elapsed_time(b)
        return out, a.elapsed_time(b)

    count = torch.zeros(nv, dtype=torch.int32, device=dev)
    span("count", lambda: _lib.check(lib.cds_mesh_adj_count(faces.data_ptr(), nf, nv, count.data_ptr(), stream), "count"))

    def offsets():
        start = torch.zeros(nv + 1, dtype=torch.int32, device=dev)
        start[1:] = torch.cumsum(count, 0, dtype=torch.int32)
        return start, torch.nonzero(count > mesh.ADJ_SMALL).reshape(-1), int(start[-1])
    (start, long_ones, ne), _ = span("offsets", offsets)
    nbr = torch.empty(ne, dtype=torch.int32, device=dev)
    cursor = torch.zeros(nv, dtype=torch.int32, device=dev)
    span("fill", lambda: _lib.check(lib.cds_mesh_adj_fill(faces.data_ptr(), nf, nv, start.data_ptr(), cursor.data_ptr(), nbr.data_ptr(),
                                                          ne, stream), "fill"))

    def long_sort():
        if long_ones.numel():
            lens = count[long_ones].long()
            owner = torch.repeat_interleave(torch.arange(long_ones.numel(), device=dev), lens)
            first = torch.cumsum(lens, 0) - lens
            at = start[long_ones].long()[owner] + (torch.arange(owner.numel(), device=dev) - first[owner])
            nbr[at] = (torch.sort((owner << 32) | nbr[at].long()).values & 0xffffffff).to(torch.int32)
    span("long", long_sort)
    deg = torch.empty(nv, dtype=torch.int32, device=dev)
    flags = torch.empty(nv, dtype=torch.uint8, device=dev)
    span("finish", lambda: _lib.check(lib.cds_mesh_adj_finish(nv, start.data_ptr(), nbr.data_ptr(), ne, deg.data_ptr(), flags.data_ptr(),
                                                              stream), "finish"))
    bufs = [torch.empty_like(vert), torch.empty_like(vert)]
    src, steps, k = vert, [], 0
    for _ in range(iterations):
        for factor in (lam, mu):
            dst = bufs[k % 2]
            _, t = span(None, lambda: _lib.check(lib.cds_mesh_smooth_step_f32(src.data_ptr(), dst.data_ptr(), nv, start.data_ptr(),
                                                                              deg.data_ptr(), nbr.data_ptr(), factor, stream), "step"))
            steps.append(t)
            src, k = dst, k + 1
    move2 = torch.empty(nv, dtype=torch.float64, device=dev)
    clamped = torch.empty(nv, dtype=torch.uint8, device=dev)
    _, limit = span(None, lambda: _lib.check(lib.cds_mesh_smooth_limit_f32(vert.data_ptr(), src.data_ptr(), nv, 0.0, move2.data_ptr(),
                                                                           clamped.data_ptr(), stream), "limit"))
    shape = {"entries": ne, "degrees": int(deg.sum(dtype=torch.int64)), "largest": int(deg.max()), "long": int(long_ones.numel()),
             "longest": int(count.max())}
    return ms, steps, limit, src, shape


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--h", type=int, default=864)
    ap.add_argument("--w", type=int, default=1152)
    ap.add_argument("--voxel", type=float, default=0.35)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--cell", type=float, default=2.0, help="cell side, in voxels, of the simplify_mesh run the table compares with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--write", default=None, help="markdown file to record the result in")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_smooth.py needs the GPU: nothing is measured without one")
    depths, masks, images, cams, points = make_scan(args.views, args.h, args.w)
    vol = mesh.TsdfVolume(points, args.voxel)
    vol.integrate(depths, masks.to(torch.uint8), images, cams)
    m = vol.extract(2)
    del vol, points, images, depths, masks
    torch.cuda.empty_cache()
    nv, nf = int(m["vertices"].shape[0]), int(m["faces"].shape[0])
    print(f"mesh: {nv} vertices, {nf} faces", flush=True)
    lib = _lib.load()
    lam, mu = 0.5, -0.53

    got, info = mesh.smooth_mesh(m, args.iterations, lam, mu)              # the check, and the warm-up of the torch steps
    _, _, _, pos, shape = timed_smooth(lib, m, args.iterations, lam, mu)
    if not torch.equal(got["vertices"].view(torch.int32), pos.view(torch.int32)):
        raise SystemExit("the step-by-step copy differs from smooth_mesh")
    del got, pos
    t = {k: [] for k in BUILD + ("step", "limit", "smooth_mesh", "simplify_mesh")}
    cell = args.cell * args.voxel
    mesh.simplify_mesh(m, cell)                                            # warm-up
    for _ in range(args.rounds):
        ms, steps, limit, pos, shape = timed_smooth(lib, m, args.iterations, lam, mu)
        del pos
        for k in BUILD:
            t[k].append(ms[k])
        t["step"] += steps
        t["limit"].append(limit)
        for name, fn in (("smooth_mesh", lambda: mesh.smooth_mesh(m, args.iterations, lam, mu)),
                         ("simplify_mesh", lambda: mesh.simplify_mesh(m, cell))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3)
    floor_bytes = nv * (12 + 8 + 12 + 12) + 4 * shape["degrees"]
    nbytes = {"count": nf * 12 + 6 * nf * 4, "offsets": nv * (4 + 4 + 4 + 1), "fill": nf * 12 + 6 * nf * (4 + 4 + 4),
              "long": 0, "finish": nv * (8 + 4 + 1) + shape["entries"] * 4 + shape["degrees"] * 4, "step": floor_bytes,
              "limit": nv * (12 + 12 + 8 + 1)}
    step_ms, simp_ms, whole = float(np.median(t["step"])), float(np.median(t["simplify_mesh"])), float(np.median(t["smooth_mesh"]))
    build_ms = sum(float(np.median(t[k])) for k in BUILD)
    lines = [f"## One scan: the mesh of {args.views} views of {args.w}x{args.h} at voxel {args.voxel}\n",
             f"{nv} vertices and {nf} faces; {shape['entries']} adjacency entries, {shape['degrees']} neighbours after rule 3 (largest "
             f"valence {shape['largest']}), {shape['long']} segments longer than {mesh.ADJ_SMALL} entries (the longest has "
             f"{shape['longest']}).  `smooth_mesh(iterations={args.iterations})`: {info}\n",
             "| step | median ms | min | max | GB it cannot avoid | fraction of 6.3 TB/s |\n|---|---|---|---|---|---|"]
    for k in BUILD + ("step", "limit"):
        med = float(np.median(t[k]))
        floor = nbytes[k] / (STREAM_TBS * 1e12) * 1e3
        label = {"step": f"step, one launch of {2 * args.iterations}", "long": "long (torch sort)"}.get(k, k)
        lines.append(f"| {label} | {stats(t[k])} | {nbytes[k] / 1e9:.3f} | {floor / med if med > 0 else 0.0:.2f} |")
    lines += [f"| adjacency build, sum of its steps | {build_ms:.3f} | | | | |",
              f"| {2 * args.iterations} step launches, sum of the medians | {2 * args.iterations * step_ms:.3f} | | | | |",
              f"| smooth_mesh({args.iterations}), host clock | {stats(t['smooth_mesh'])} | | |",
              f"| simplify_mesh(cell {args.cell:g} voxels, quadric), host clock | {stats(t['simplify_mesh'])} | | |\n",
              f"One step launch is {step_ms / simp_ms:.3f} of `simplify_mesh` on this mesh; the whole `smooth_mesh({args.iterations})` is "
              f"{whole / simp_ms:.2f} of it.  The step's floor is {floor_bytes / 1e9:.3f} GB = "
              f"{floor_bytes / (STREAM_TBS * 1e12) * 1e3:.3f} ms at 6.3 TB/s.\n"]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Smoothing of a scan's mesh on the MI355X (`csrc/mesh_smooth.hip`)\n\n"
                    f"`python scripts/time_mesh_smooth.py --views {args.views} --h {args.h} --w {args.w} --voxel {args.voxel} --iterations "
                    f"{args.iterations} --cell {args.cell:g} --rounds {args.rounds}`: {args.rounds} repetitions after a warm-up, one "
                    "process, one MI355X.  Steps between HIP events with a synchronise after each, smooth_mesh and simplify_mesh by the "
                    "host clock around a device synchronise.  No threshold: nothing before this does the step.  Recorded values.\n\n" +
                    text +
                    "\n## Reading the table\n\n"
                    "- `step` is one thread per vertex: a lane gathers its neighbours' rows, 12 bytes each from wherever the extraction "
                    "put them, and adds them in one serial fp64 chain per coordinate.  The floor counts every row once; what the "
                    "kernel moves beyond it is rows gathered again by the other vertices around them, which come from cache when the "
                    "neighbours lie close in the vertex order, and its time also grows with the largest valence of a wave.\n"
                    "- `count` and `fill` are one thread per face with two integer atomics per edge slot; `fill` also scatters the "
                    "entries.  `offsets` holds the one host read of the build.\n"
                    "- `finish` sorts a segment in place in global memory, one thread per vertex.\n"
                    "\n## Not measured\n\n"
                    "- The gathers of a vertex spread over several lanes with the chain kept in order, against this one thread per vertex.\n"
                    "- The vertices renumbered along a space-filling curve before the iterations, so that more gathers hit the cache.\n"
                    "- The adjacency from a global sort of packed (i, j) keys, against the counting build.\n")
        print(f"wrote {args.write}", flush=True)


if __name__ == "__main__":
    main()
