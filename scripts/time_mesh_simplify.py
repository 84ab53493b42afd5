"""Time the simplification of csrc/mesh_simplify.hip on a DTU-shaped scan: the mesh of scripts/time_mesh_clean.py.

    python scripts/time_mesh_simplify.py [--views 49 --h 864 --w 1152 --voxel 0.35] [--pieces 4000] [--cells 2,4,8] [--rounds 3]
        [--write profiles/mesh_simplify.md]

The scan and its mesh: time_mesh_clean's (time_tsdf_mesh.render fused and extracted by mesh.TsdfVolume at --voxel, --pieces
tetrahedra put in at seeded places).  For each cell of --cells voxels and both placements, mesh.simplify_mesh is first held to
the step-by-step copy below (the same arrays, bit for bit) and then timed.

Reported, each a median with minimum and maximum over --rounds after a warm-up, one process:
  cells / assign / merge / faces / incidences / quadric / duplicates / mark / offsets / gather
                   the steps of mesh.simplify_mesh between HIP events, kernels through the C entry points: the cells of
                   pointcloud.voxel_groups (keys, a stable sort, the runs), the cluster of every vertex, cds_voxel_merge_f32, the
                   face pass, the incidence lists (a stable sort of the 3 F corner clusters and the offsets; quadric only), the
                   quadric kernel, the duplicates (the packed identities of the faces that did not collapse, a stable sort, the
                   first of each run), mark, the two cumsums, gather
  simplify_mesh    the whole call by the host clock around a device synchronise
  clean_mesh       mesh.clean_mesh(min_faces = 100) on the same mesh in the same run, by the same clock: the sibling of known cost
With each step the bytes it cannot avoid, computed from the shapes (below), and the fraction of the 6.3 TB/s a streaming kernel
reaches on the MI355X that they are of its time; a sort is counted as one pass over its keys in and its keys and indices out.
Also the largest cluster's incidence count, because the sums of a cluster are one thread's serial chain.  Recorded values, not
thresholds.  There is no CPU fallback: without a GPU the script fails."""
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
from cds_mvsnet_amd.pointcloud import pack_colors, voxel_groups  # noqa: E402
from time_mesh_clean import add_debris  # noqa: E402
from time_tsdf_mesh import STREAM_TBS, render as make_scan, stats  # noqa: E402

STEPS = ("cells", "assign", "merge", "faces", "incidences", "quadric", "duplicates", "mark", "offsets", "gather")


def timed_simplify(lib, m, cell, placement):
    """simplify_mesh's steps with an event between them -> ({step: ms}, shape counts for the byte model, the mesh)."""
    vert, col, faces = m["vertices"], m["colors"], m["faces"]
    nv, nf, dev = vert.shape[0], faces.shape[0], vert.device
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

    perm, start, ukeys, counts = span("cells", lambda: voxel_groups(vert, cell, "time_mesh_simplify"))
    nc = int(ukeys.numel())

    def assign():
        cluster = torch.empty(nv, dtype=torch.int32, device=dev)
        cluster[perm] = torch.repeat_interleave(torch.arange(nc, dtype=torch.int32, device=dev), counts, output_size=nv)
        return cluster
    cluster = span("assign", assign)
    mean = torch.empty((nc, 3), dtype=torch.float32, device=dev)
    packed = torch.empty(nc, dtype=torch.int32, device=dev)
    members = torch.empty(nc, dtype=torch.int32, device=dev)
    span("merge", lambda: _lib.check(lib.cds_voxel_merge_f32(vert.data_ptr(), pack_colors(col).data_ptr(), None, nv, perm.data_ptr(),
                                                             start.data_ptr(), nc, mean.data_ptr(), packed.data_ptr(), None,
                                                             members.data_ptr(), stream), "merge"))
    fclus = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    ident = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    gone = torch.empty(nf, dtype=torch.uint8, device=dev)
    span("faces", lambda: _lib.check(lib.cds_mesh_simplify_faces(faces.data_ptr(), nf, nv, cluster.data_ptr(), nc, fclus.data_ptr(),
                                                                 gone.data_ptr(), ident.data_ptr(), stream), "faces"))
    pos, n_fell, largest = mean, 0, 0
    if placement == "quadric":
        def incidences():
            owner, inc = torch.sort(fclus.reshape(-1), stable=True)
            return inc, torch.searchsorted(owner, torch.arange(nc + 1, dtype=torch.int32, device=dev)).to(torch.int32)
        inc, inc_start = span("incidences", incidences)
        pos = torch.empty((nc, 3), dtype=torch.float32, device=dev)
        fell = torch.empty(nc, dtype=torch.uint8, device=dev)
        span("quadric", lambda: _lib.check(lib.cds_mesh_simplify_quadric_f32(vert.data_ptr(), nv, faces.data_ptr(), nf, perm.data_ptr(),
                                                                             start.data_ptr(), inc.data_ptr(), inc_start.data_ptr(), nc,
                                                                             cell, pos.data_ptr(), fell.data_ptr(), stream), "quadric"))
        n_fell, largest = int(fell.sum()), int((inc_start[1:] - inc_start[:-1]).max())
        del inc, inc_start

    def duplicates():
        alive = torch.nonzero(gone == 0).reshape(-1)
        fkeep = torch.zeros(nf, dtype=torch.uint8, device=dev)
        if alive.numel():
            fkeep[alive[mesh._first_of_identity(ident[alive].long(), nc)]] = 1
        return fkeep, int(alive.numel())
    fkeep, n_alive = span("duplicates", duplicates)
    ckeep = torch.zeros(nc, dtype=torch.uint8, device=dev)
    span("mark", lambda: _lib.check(lib.cds_mesh_simplify_mark(fclus.data_ptr(), fkeep.data_ptr(), nf, nc, ckeep.data_ptr(), stream),
                                    "mark"))

    def offsets():
        cend, fend = torch.cumsum(ckeep, 0, dtype=torch.int64), torch.cumsum(fkeep, 0, dtype=torch.int64)
        return (cend - ckeep).to(torch.int32), (fend - fkeep).to(torch.int32), int(cend[-1]), int(fend[-1])
    cnew, fnew, nv_out, nf_out = span("offsets", offsets)
    out = {"vertices": torch.empty((nv_out, 3), dtype=torch.float32, device=dev),
           "colors": torch.empty((nv_out, 3), dtype=torch.uint8, device=dev),
           "faces": torch.empty((nf_out, 3), dtype=torch.int32, device=dev)}
    span("gather", lambda: _lib.check(lib.cds_mesh_simplify_gather(pos.data_ptr(), packed.data_ptr(), nc, ckeep.data_ptr(),
                                                                   cnew.data_ptr(), fclus.data_ptr(), nf, fkeep.data_ptr(),
                                                                   fnew.data_ptr(), nv_out, nf_out, out["vertices"].data_ptr(),
                                                                   out["colors"].data_ptr(), out["faces"].data_ptr(), stream), "gather"))
    shape = {"nc": nc, "alive": n_alive, "nv_out": nv_out, "nf_out": nf_out, "fallback": n_fell, "largest": largest}
    return ms, shape, out


def step_bytes(nv, nf, s, placement):
    """The bytes a step cannot avoid, from the shapes."""
    nc, na, vo, fo = s["nc"], s["alive"], s["nv_out"], s["nf_out"]
    quadric = placement == "quadric"
    return {"cells": nv * (12 + 8) + nv * (8 + 8 + 8) + nv * 8,            # keys from positions; the sort; the runs
            "assign": nc * 8 + nv * (4 + 8 + 4),                          # counts; the cluster of a sorted place, perm, the scatter
            "merge": nv * (8 + 12 + 3) + nv * 4 + nc * (4 + 12 + 4 + 4),  # perm, position, colour, the packed colours; the rows out
            "faces": nf * (12 + 12 + 12 + 12 + 1),                        # indices, their clusters; clusters, identity, flag out
            "incidences": 3 * nf * (4 + 4 + 8) if quadric else 0,         # the sort's keys in, keys and indices out
            "quadric": (3 * nf * (8 + 12 + 36) + nv * (8 + 12) + nc * (8 + 13)) if quadric else 0,
            "duplicates": nf * (1 + 1) + na * (8 + 12 + 8) + na * (8 + 8 + 8) + na * 8,   # flags; identities to keys; the sort; the runs
            "mark": nf * 1 + fo * 12 + nc,
            "offsets": (nc + nf) * (1 + 8 + 4),
            "gather": nc * (1 + 4) + vo * (12 + 4 + 15) + nf * (1 + 4) + fo * (12 + 12 + 12)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--h", type=int, default=864)
    ap.add_argument("--w", type=int, default=1152)
    ap.add_argument("--voxel", type=float, default=0.35)
    ap.add_argument("--pieces", type=int, default=4000)
    ap.add_argument("--cells", default="2,4,8", help="cell sides in voxels")
    ap.add_argument("--min_faces", type=int, default=100, help="of the clean_mesh run the table compares with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--write", default=None, help="markdown file to record the result in")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_simplify.py needs the GPU: nothing is measured without one")
    depths, masks, images, cams, points = make_scan(args.views, args.h, args.w)
    vol = mesh.TsdfVolume(points, args.voxel)
    vol.integrate(depths, masks.to(torch.uint8), images, cams)
    scan = vol.extract(2)
    del vol, points, images, depths, masks
    m = add_debris(scan, args.pieces)
    del scan
    torch.cuda.empty_cache()
    nv, nf = int(m["vertices"].shape[0]), int(m["faces"].shape[0])
    print(f"mesh: {nv} vertices, {nf} faces", flush=True)
    lib = _lib.load()

    clean = []
    mesh.clean_mesh(m, args.min_faces)                                     # warm-up
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh.clean_mesh(m, args.min_faces)
        torch.cuda.synchronize()
        clean.append((time.perf_counter() - t0) * 1e3)
    clean_ms = float(np.median(clean))
    print(f"clean_mesh(min_faces={args.min_faces}): {stats(clean)} ms", flush=True)

    lines = [f"## One scan: the mesh of {args.views} views of {args.w}x{args.h} at voxel {args.voxel}, with {args.pieces} tetrahedra put in\n",
             f"{nv} vertices and {nf} faces.  `clean_mesh(min_faces={args.min_faces})` on this mesh in this run, host clock: "
             f"{stats(clean)} ms (median | min | max).\n"]
    summary = ["| cell, voxels | placement | vertices | faces | clusters | collapsed | duplicates | fallbacks | largest cluster, "
               "incidences | simplify_mesh ms | of clean_mesh |\n|---|---|---|---|---|---|---|---|---|---|---|"]
    for cv in (float(x) for x in args.cells.split(",")):
        cell = cv * args.voxel
        for placement in mesh.PLACEMENTS:
            got, info = mesh.simplify_mesh(m, cell, placement)             # the check, and the warm-up of the torch steps
            _, shape, out = timed_simplify(lib, m, cell, placement)
            for k in ("vertices", "colors", "faces"):
                if not torch.equal(got[k].view(torch.uint8), out[k].view(torch.uint8)):
                    raise SystemExit(f"the step-by-step copy differs from simplify_mesh in {k} (cell {cell}, {placement})")
            del got, out
            t = {k: [] for k in STEPS + ("simplify_mesh",)}
            for _ in range(args.rounds):
                ms, shape, out = timed_simplify(lib, m, cell, placement)
                del out
                for k in STEPS:
                    t[k].append(ms[k])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mesh.simplify_mesh(m, cell, placement)
                torch.cuda.synchronize()
                t["simplify_mesh"].append((time.perf_counter() - t0) * 1e3)
            nbytes = step_bytes(nv, nf, shape, placement)
            whole = float(np.median(t["simplify_mesh"]))
            summary.append(f"| {cv:g} | {placement} | {info['vertices'][1]} | {info['faces'][1]} | {info['clusters']} | "
                           f"{info['collapsed']} | {info['duplicates']} | {info['fallback']} | "
                           f"{shape['largest'] if placement == 'quadric' else ''} | {whole:.2f} | {whole / clean_ms:.2f} |")
            lines += [f"### Cell {cv:g} voxels = {cell:g}, {placement}\n", f"{info}\n",
                      "| step | median ms | min | max | GB it cannot avoid | fraction of 6.3 TB/s |\n|---|---|---|---|---|---|"]
            for k in STEPS:
                med = float(np.median(t[k]))
                floor = nbytes[k] / (STREAM_TBS * 1e12) * 1e3
                lines.append(f"| {k} | {stats(t[k])} | {nbytes[k] / 1e9:.3f} | {floor / med if med > 0 else 0.0:.2f} |")
            lines.append(f"| sum of the steps | {sum(float(np.median(t[k])) for k in STEPS):.3f} | | | | |")
            lines.append(f"| simplify_mesh, host clock | {stats(t['simplify_mesh'])} | | |\n")
            print("\n".join(lines[-(len(STEPS) + 6):]), flush=True)
            torch.cuda.empty_cache()
    text = "\n".join(lines[:2] + summary + [""] + lines[2:])
    print("\n".join(summary), flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Simplification of a scan's mesh on the MI355X (`csrc/mesh_simplify.hip`)\n\n"
                    f"`python scripts/time_mesh_simplify.py --views {args.views} --h {args.h} --w {args.w} --voxel {args.voxel} --pieces "
                    f"{args.pieces} --cells {args.cells} --rounds {args.rounds}`: {args.rounds} repetitions after a warm-up, one process, "
                    "one MI355X.  Steps between HIP events with a synchronise after each, simplify_mesh and clean_mesh by the host "
                    "clock around a device synchronise.  No threshold: nothing before this does the step.  Recorded values.\n\n" + text +
                    "\n## Reading the tables\n\n"
                    "- `cells` is `pointcloud.voxel_groups` as `--merge_voxel` runs it: a key per vertex, a stable sort of V int64 "
                    "keys, the runs, and the bounding box read back on the host.  It is the largest step at every cell.\n"
                    "- `faces` counts one cluster word per corner; the words of neighbouring faces come from cache, so its "
                    "fraction can pass 1.\n"
                    "- `quadric` is one thread per cluster: its time is gathers (56 bytes per incidence from three arrays) and "
                    "nine serial fp64 chains, and it grows with the largest cluster of a wave, not with the streamed bytes.\n"
                    "- `incidences` and `duplicates` are torch sorts (3 F int32 keys; the int64 identities of the faces that did "
                    "not collapse).\n"
                    "\n## Not measured\n\n"
                    "- The quadric sums with a cluster's gathers and cross products spread across a wave and the nine chains kept "
                    "in order, against this one thread per cluster.\n"
                    "- The duplicates through a device table and `atomicMin` on the face index, against the stable sort.\n"
                    "- The incidence lists from a counting pass over the faces instead of a sort of the 3 F corner clusters.\n")
        print(f"wrote {args.write}", flush=True)


if __name__ == "__main__":
    main()
