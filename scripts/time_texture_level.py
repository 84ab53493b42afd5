"""Time the seam levelling of csrc/mesh_texture.hip on the DTU-shaped scan of scripts/time_mesh_texture.py.

    python scripts/time_texture_level.py [--views 49 --h 864 --w 1152 --voxel 0.35] [--pieces 4000] [--cells 2,4,8] [--level 20]
        [--rounds 3] [--write profiles/texture_level.md]

The scan and its mesh are time_mesh_texture's; every view's image gets its own grey offset in -20 .. 20 levels, so that the seams
carry exposure steps.  The mesh is simplified at each cell of --cells voxels and textured.  texture.texture_mesh(level=1) is first
held to the step-by-step copy below (sample, ok, g, atlas, bit for bit) and then timed.

Reported, each a median with minimum and maximum over --rounds after a warm-up, one process:
  nodes, torch              rule L1: texture.level_nodes (nonzero, unique, a stable sort, bincount, cumsum), host clock
  node samples              cds_texture_level_samples
  pair table                cds_texture_level_pairs with its spans (torch.unique_consecutive before the launch), host clock
  one step                  cds_texture_level_step, the mean of 20 launches between two events
  fill / levelled fill      cds_texture_fill and cds_texture_fill_level on the same tables, alternating
  texture_mesh, level 0 / N the whole call by the host clock around a device synchronise
kernels between HIP events through the C entry points.  With the step the bytes it gathers and the time they would take at the
6.3 TB/s a streaming kernel reaches on the MI355X.  Recorded values, not thresholds.  There is no CPU fallback: without a GPU the
script fails."""
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

STEPS = ("nodes, torch", "node samples", "pair table", "one step", "fill", "levelled fill")
CHUNK = 8
STEP_LAUNCHES = 20


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def timed_level(lib, m, images, tab, tex, lam, max_cell):
    """The steps of levelling on the view and cell tables of an unlevelled texture_mesh -> ({step: ms}, tensors, gather bytes)."""
    vert, col, faces = m["vertices"], m["colors"], m["faces"]
    nv, nf, dev = int(vert.shape[0]), int(faces.shape[0]), vert.device
    v, h, w = (int(x) for x in images.shape[:3])
    stream = torch.cuda.current_stream().cuda_stream
    views = torch.tensor([(3 * h * w * k, h, w) for k in range(v)], dtype=torch.int64).to(dev)
    ms = {}
    ms["nodes, torch"], nodes = host_ms(lambda: texture.level_nodes(faces, tex["view"], v))
    key, cnode, clist, cstart = (nodes[k] for k in ("node_key", "corner_node", "corner_list", "corner_start"))
    n = int(key.numel())
    sample = torch.empty((n, 3), dtype=torch.float64, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    ms["node samples"], _ = event_ms(lambda: _lib.check(lib.cds_texture_level_samples(
        vert.data_ptr(), nv, tab.data_ptr(), images.data_ptr(), int(images.numel()), views.data_ptr(), v, key.data_ptr(), n,
        sample.data_ptr(), ok.data_ptr(), stream), "samples"))
    ms["pair table"], (table, span, longest) = host_ms(lambda: texture.level_pair_table(key, sample, ok, v))
    host = torch.cat([table.reshape(-1), torch.bincount(key % v, minlength=v)]).cpu().numpy()
    pair = host[:4 * v * v].reshape(v, v, 4)
    offsets = torch.from_numpy(texture.level_offsets(pair[:, :, 0], pair[:, :, 1:], host[4 * v * v:])).to(dev)
    g0 = offsets[key % v].contiguous()
    g1, g2 = torch.empty_like(g0), torch.empty_like(g0)

    def steps():
        a, b = g0, g1
        for _ in range(STEP_LAUNCHES):
            _lib.check(lib.cds_texture_level_step(sample.data_ptr(), ok.data_ptr(), span.data_ptr(), cstart.data_ptr(), clist.data_ptr(),
                                                  int(clist.numel()), cnode.data_ptr(), n, nf, v, lam, a.data_ptr(), b.data_ptr(),
                                                  stream), "step")
            a, b = b, (g2 if b is g1 else g1)
    t, _ = event_ms(steps)
    ms["one step"] = t / STEP_LAUNCHES
    _lib.check(lib.cds_texture_level_step(sample.data_ptr(), ok.data_ptr(), span.data_ptr(), cstart.data_ptr(), clist.data_ptr(),
                                          int(clist.numel()), cnode.data_ptr(), n, nf, v, lam, g0.data_ptr(), g1.data_ptr(), stream),
               "step")                                                # g1: one iteration from the offsets, what level=1 gives
    # the fills on the tables texture_mesh builds between its launches
    c = tex["cell"][:, 2].to(torch.int64)
    order = torch.sort(-c, stable=True).indices
    units = (c[order] >> 2) ** 2
    ends = torch.cumsum(units, 0)
    starts, total = ends - units, int(ends[-1])
    ah, aw = (int(x) for x in tex["atlas"].shape[:2])
    atlas = [torch.empty((ah, aw, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    fill = (vert.data_ptr(), col.data_ptr(), nv, faces.data_ptr(), nf, tab.data_ptr(), images.data_ptr(), int(images.numel()),
            views.data_ptr(), v, tex["view"].data_ptr(), tex["cell"].data_ptr(), order.data_ptr(), starts.data_ptr(), total, max_cell, ah, aw)
    ms["fill"], _ = event_ms(lambda: _lib.check(lib.cds_texture_fill(*fill, atlas[0].data_ptr(), texture.FILL_PER_UNIT, stream), "fill"))
    ms["levelled fill"], _ = event_ms(lambda: _lib.check(lib.cds_texture_fill_level(
        *fill, atlas[1].data_ptr(), texture.FILL_PER_UNIT, cnode.data_ptr(), g1.data_ptr(), n, stream), "levelled fill"))
    # what one step reads and writes: per node its own g, sample, ok, span and list range, and the new g; per other node of the
    # vertex a sample, a g and an ok; per corner its list entry and two partners' node and g
    others = int((span[:, 1].to(torch.int64) - 1).sum())
    gather = n * (24 + 24 + 1 + 8 + 16 + 24) + others * (24 + 24 + 1) + int(clist.numel()) * (8 + 2 * (4 + 24))
    seam_nodes = int((span[:, 1] > 1).sum())
    return ms, {"sample": sample, "ok": ok, "g": g1, "atlas": atlas, "nodes": n, "pairs": int(pair[:, :, 0].sum()),
                "seam_nodes": seam_nodes, "longest": int(longest)}, gather


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--h", type=int, default=864)
    ap.add_argument("--w", type=int, default=1152)
    ap.add_argument("--voxel", type=float, default=0.35)
    ap.add_argument("--pieces", type=int, default=4000)
    ap.add_argument("--cells", default="2,4,8", help="simplification cell sides in voxels")
    ap.add_argument("--level", type=int, default=20)
    ap.add_argument("--level_lambda", type=float, default=0.1)
    ap.add_argument("--max_cell", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--write", default=None, help="markdown file to record the result in")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_texture_level.py needs the GPU: nothing is measured without one")
    depths, masks, images, cams, points = make_scan(args.views, args.h, args.w)
    vol = mesh.TsdfVolume(points, args.voxel)
    vol.integrate(depths, masks.to(torch.uint8), images, cams)
    scan = vol.extract(2)
    del vol, points, depths, masks
    m = add_debris(scan, args.pieces)
    del scan
    # every view under its own exposure: a grey offset in -20 .. 20 levels
    shift = torch.tensor([(37 * k) % 41 - 20 for k in range(args.views)], dtype=torch.int16, device=images.device)
    images = (images.to(torch.int16) + shift[:, None, None, None]).clamp_(0, 255).to(torch.uint8).contiguous()
    torch.cuda.empty_cache()
    print(f"mesh: {int(m['vertices'].shape[0])} vertices, {int(m['faces'].shape[0])} faces", flush=True)
    lib = _lib.load()
    tab = render.camera_table(cams).cuda()
    lines = []
    summary = ["| cell, voxels | faces | nodes | nodes at seams | seam pairs | most labels at a vertex | mean jump before -> after | "
               f"texture_mesh ms | with level {args.level} ms |\n|---|---|---|---|---|---|---|---|---|"]
    for cv in (float(x) for x in args.cells.split(",")):
        sm, _ = mesh.simplify_mesh(m, cv * args.voxel, "quadric")
        kw = dict(max_cell=args.max_cell, chunk=CHUNK)
        tex, _ = texture.texture_mesh(sm, images, cams, **kw)
        one, _ = texture.texture_mesh(sm, images, cams, level=1, level_lambda=args.level_lambda, **kw)      # the check, the warm-up
        _, got, _ = timed_level(lib, sm, images, tab, tex, args.level_lambda, args.max_cell)
        for k in ("sample", "ok", "g"):
            if not torch.equal(got[k], one["level"][k]):
                raise SystemExit(f"the step-by-step copy differs from texture_mesh in {k} (cell {cv})")
        if not torch.equal(got["atlas"][0], tex["atlas"]) or not torch.equal(got["atlas"][1], one["atlas"]):
            raise SystemExit(f"the step-by-step copy differs from texture_mesh in an atlas (cell {cv})")
        _, info = texture.texture_mesh(sm, images, cams, level=args.level, level_lambda=args.level_lambda, **kw)
        del one
        t = {k: [] for k in STEPS + ("texture_mesh", "levelled")}
        for _ in range(args.rounds):
            ms, got, gather = timed_level(lib, sm, images, tab, tex, args.level_lambda, args.max_cell)
            for k in STEPS:
                t[k].append(ms[k])
            t["texture_mesh"].append(host_ms(lambda: texture.texture_mesh(sm, images, cams, **kw))[0])
            t["levelled"].append(host_ms(lambda: texture.texture_mesh(sm, images, cams, level=args.level,
                                                                      level_lambda=args.level_lambda, **kw))[0])
        med = {k: float(np.median(t[k])) for k in t}
        nf = info["faces"]
        floor = gather / (STREAM_TBS * 1e12) * 1e3
        pairs, before, after = info["seam"]
        summary.append(f"| {cv:g} | {nf} | {got['nodes']} | {got['seam_nodes']} | {pairs} | {got['longest']} | {before:.2f} -> {after:.2f} | "
                       f"{med['texture_mesh']:.2f} | {med['levelled']:.2f} |")
        lines += [f"### Simplified at {cv:g} voxels: {nf} faces, {got['nodes']} nodes\n", f"{info}\n",
                  "| step | median ms | min | max |\n|---|---|---|---|"]
        lines += [f"| {k} | {stats(t[k])} |" for k in STEPS]
        lines.append(f"| texture_mesh, host clock | {stats(t['texture_mesh'])} |")
        lines.append(f"| texture_mesh with level {args.level}, host clock | {stats(t['levelled'])} |\n")
        lines.append(f"One step gathers {gather / 1e6:.1f} MB: {floor:.4f} ms to stream at {STREAM_TBS} TB/s; it takes "
                     f"{med['one step'] / floor:.1f} times that.  The levelled fill takes {med['levelled fill'] / med['fill']:.3f} times the "
                     f"plain fill; the g of a face's three corner nodes are {72 * nf / 1e6:.1f} MB, "
                     f"{72 * nf / (STREAM_TBS * 1e12) * 1e3:.4f} ms to stream.\n")
        print("\n".join(lines[-(len(STEPS) + 8):]), flush=True)
        del sm, tex, got
        torch.cuda.empty_cache()
    print("\n".join(summary), flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Levelling the seams of a scan's texture on the MI355X (`csrc/mesh_texture.hip`)\n\n"
                    f"`python scripts/time_texture_level.py --views {args.views} --h {args.h} --w {args.w} --voxel {args.voxel} --pieces "
                    f"{args.pieces} --cells {args.cells} --level {args.level} --rounds {args.rounds}`: {args.rounds} repetitions after a "
                    "warm-up, one process, one MI355X.  Kernels between HIP events with a synchronise after each, the torch steps and "
                    "texture_mesh by the host clock around a device synchronise.  Every view carries a grey offset in -20 .. 20 "
                    "levels.  No threshold: nothing before this does the step.  Recorded values.\n\n"
                    + "\n".join(summary) + "\n\n" + "\n".join(lines) + "\n")
        print(f"wrote {args.write}", flush=True)


if __name__ == "__main__":
    main()
