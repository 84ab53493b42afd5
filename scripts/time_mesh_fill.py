"""Time the hole filling of csrc/mesh_fill.hip on a DTU-shaped scan: the mesh of scripts/time_tsdf_mesh.py with holes punched.

    python scripts/time_mesh_fill.py [--views 49 --h 864 --w 1152 --voxel 0.35] [--holes 600] [--max_edges 64] [--rounds 3]
        [--write profiles/mesh_fill.md]

The scan and its mesh: time_tsdf_mesh.render fused and extracted by mesh.TsdfVolume at --voxel; the mesh is open, so its own rim is
there.  Into it --holes holes of each of six kinds are punched at seeded random places: one face (3 edges), and the faces within
0, 2, 4, 6 and 9 rings of a vertex (rims of about 6, 18, 30, 42 and 60 edges where the valence is 6).  mesh.fill_holes is first
held to the step-by-step copy below (the same mesh, bit for bit) and then timed.

Reported, each a median with minimum and maximum over --rounds after a warm-up, one process:
  keys / sort / border / init / doubling / walk / offsets / emit
                   the phases of fill_holes between HIP events, kernels through the C entry points: the key kernel, the torch
                   sort of the 3 F keys, the border kernel, the kernel of rule 3 with the border count's host read and the list of
                   regular vertices, all rounds of the pointer doubling, the walk, the prefix sums with the ONE read of the fill,
                   the copies of the input's rows with the emit kernel
  fill_holes       the whole call by the host clock around a synchronise
With the three hand-written kernels that stream (keys, border, emit with the copies) the time their bytes would take at the rate
of a device copy measured in the same run.  Recorded values, not thresholds.  There is no CPU fallback: without a GPU the script
fails."""
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
from time_tsdf_mesh import render as make_scan, stats  # noqa: E402

PHASES = ("keys", "sort", "border", "init", "doubling", "walk", "offsets", "emit")


def punch(m, holes, seed=0):
    """The mesh without the faces of 6 x holes seeded places -> (mesh dict, faces removed)."""
    faces, nv = m["faces"], int(m["vertices"].shape[0])
    nf, dev = int(faces.shape[0]), faces.device
    g = torch.Generator(device="cpu").manual_seed(seed)
    gone = torch.zeros(nf, dtype=torch.bool, device=dev)
    gone[torch.randint(0, nf, (holes,), generator=g).to(dev)] = True
    idx = faces.long()
    for rings in (0, 2, 4, 6, 9):
        sel = torch.zeros(nv, dtype=torch.bool, device=dev)
        sel[torch.randint(0, nv, (holes,), generator=g).to(dev)] = True
        for _ in range(rings):
            sel[idx[sel[idx].any(1)].reshape(-1)] = True
        gone |= sel[idx].any(1)
    return dict(m, faces=faces[~gone].contiguous()), int(gone.sum())


def copy_rate(dev, nbytes=1 << 30, rounds=5):
    """Bytes read and written per second by a device copy of nbytes."""
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst.copy_(src)
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return 2.0 * nbytes / (float(np.median(ms)) * 1e-3)


def timed_fill(lib, m, max_edges):
    """fill_holes' phases with an event between them -> ({phase: ms}, the mesh made, shape numbers)."""
    vert, col, faces = m["vertices"], m["colors"], m["faces"]
    nv, nf, dev = int(vert.shape[0]), int(faces.shape[0]), vert.device
    stream = torch.cuda.current_stream().cuda_stream
    ms = dict.fromkeys(PHASES, 0.0)

    def span(name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms[name] += a.elapsed_time(b)
        return out

    def i32(*shape, fill=None):
        return torch.empty(shape, dtype=torch.int32, device=dev) if fill is None else torch.full(shape, fill, dtype=torch.int32, device=dev)
    keys = torch.empty(3 * nf, dtype=torch.int64, device=dev)
    span("keys", lambda: _lib.check(lib.cds_mesh_fill_keys(faces.data_ptr(), nf, nv, keys.data_ptr(), stream), "keys"))
    keys = span("sort", lambda: torch.sort(keys).values)
    leave, enter, nxt, prv = i32(nv, fill=0), i32(nv, fill=0), i32(nv, fill=-1), i32(nv, fill=-1)
    span("border", lambda: _lib.check(lib.cds_mesh_fill_borders(keys.data_ptr(), 3 * nf, nv, leave.data_ptr(), enter.data_ptr(),
                                                                nxt.data_ptr(), prv.data_ptr(), stream), "borders"))
    regular = torch.empty(nv, dtype=torch.uint8, device=dev)
    pairs = [i32(2, nv) for _ in range(4)]

    def init():
        _lib.check(lib.cds_mesh_fill_init(nv, leave.data_ptr(), enter.data_ptr(), nxt.data_ptr(), prv.data_ptr(), regular.data_ptr(),
                                          *(t.data_ptr() for t in pairs), stream), "init")
        return int(leave.sum()), torch.nonzero(regular).reshape(-1).to(torch.int32)
    n_border, ring = span("init", init)
    n_ring = int(ring.numel())
    label, jump, label_b, jump_b = pairs
    rounds = (max_edges - 1).bit_length()

    def doubling():
        nonlocal label, jump, label_b, jump_b
        for _ in range(rounds):
            _lib.check(lib.cds_mesh_fill_double(ring.data_ptr(), n_ring, nv, label.data_ptr(), jump.data_ptr(), label_b.data_ptr(),
                                                jump_b.data_ptr(), stream), "double")
            label, jump, label_b, jump_b = label_b, jump_b, label, jump
    span("doubling", doubling)
    edges = i32(n_ring)
    centre = torch.empty((n_ring, 3), dtype=torch.float32, device=dev)
    centre_color = torch.empty((n_ring, 3), dtype=torch.uint8, device=dev)
    span("walk", lambda: _lib.check(lib.cds_mesh_fill_walk(vert.data_ptr(), col.data_ptr(), nv, nxt.data_ptr(), regular.data_ptr(),
                                                           label.data_ptr(), ring.data_ptr(), n_ring, max_edges, edges.data_ptr(),
                                                           centre.data_ptr(), centre_color.data_ptr(), stream), "walk"))

    def offsets():
        fan = (edges >= 4).to(torch.int64)
        made = torch.where(edges == 3, 1, edges).to(torch.int64)
        vend, fend = torch.cumsum(fan, 0), torch.cumsum(made, 0)
        counts = [int(x) for x in torch.stack([(edges > 0).sum(), vend[-1], fend[-1], edges.max().long(), edges.sum()]).cpu()]
        return counts, vend - fan, fend - made
    (loops, new_v, new_f, largest, closed), vertex_at, face_at = span("offsets", offsets)

    def emit():
        out = {"vertices": torch.empty((nv + new_v, 3), dtype=torch.float32, device=dev),
               "colors": torch.empty((nv + new_v, 3), dtype=torch.uint8, device=dev),
               "faces": torch.empty((nf + new_f, 3), dtype=torch.int32, device=dev)}
        out["vertices"][:nv].copy_(vert)
        out["colors"][:nv].copy_(col)
        out["faces"][:nf].copy_(faces)
        _lib.check(lib.cds_mesh_fill_emit(nxt.data_ptr(), regular.data_ptr(), nv, nf, ring.data_ptr(), n_ring, max_edges,
                                          edges.data_ptr(), vertex_at.data_ptr(), face_at.data_ptr(), centre.data_ptr(),
                                          centre_color.data_ptr(), new_v, new_f, out["vertices"].data_ptr(), out["colors"].data_ptr(),
                                          out["faces"].data_ptr(), stream), "emit")
        return out
    out = span("emit", emit)
    candidates = int(((label[0][ring.long()] == ring) & (label[1][ring.long()] == ring)).sum())
    hist = torch.bincount(edges[edges > 0].long(), minlength=max_edges + 1).cpu().numpy()
    shape = {"border": n_border, "regular": n_ring, "candidates": candidates, "rounds": rounds, "loops": loops, "largest": largest,
             "closed": closed, "new_v": new_v, "new_f": new_f, "hist": hist}
    return ms, out, shape


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--h", type=int, default=864)
    ap.add_argument("--w", type=int, default=1152)
    ap.add_argument("--voxel", type=float, default=0.35)
    ap.add_argument("--holes", type=int, default=600, help="holes punched of each of the six kinds")
    ap.add_argument("--max_edges", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--write", default=None, help="markdown file to record the result in")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_fill.py needs the GPU: nothing is measured without one")
    depths, masks, images, cams, points = make_scan(args.views, args.h, args.w)
    vol = mesh.TsdfVolume(points, args.voxel)
    vol.integrate(depths, masks.to(torch.uint8), images, cams)
    m = vol.extract(2)
    del vol, points, images, depths, masks
    torch.cuda.empty_cache()
    m, removed = punch(m, args.holes)
    nv, nf = int(m["vertices"].shape[0]), int(m["faces"].shape[0])
    print(f"mesh: {nv} vertices, {nf} faces after {removed} were punched out", flush=True)
    lib = _lib.load()
    rate = copy_rate(m["vertices"].device)

    got, info = mesh.fill_holes(m, args.max_edges)                         # the check, and the warm-up of the torch steps
    _, out, shape = timed_fill(lib, m, args.max_edges)
    if not all(torch.equal(got[k].view(torch.uint8), out[k].view(torch.uint8)) for k in got):
        raise SystemExit("the step-by-step copy differs from fill_holes")
    del got, out
    t = {k: [] for k in PHASES + ("fill_holes",)}
    for _ in range(args.rounds):
        ms, out, shape = timed_fill(lib, m, args.max_edges)
        del out
        for k in PHASES:
            t[k].append(ms[k])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh.fill_holes(m, args.max_edges)
        torch.cuda.synchronize()
        t["fill_holes"].append((time.perf_counter() - t0) * 1e3)
    nbytes = {"keys": nf * (12 + 24), "border": 3 * nf * 8 + shape["border"] * 16,
              "emit": 2 * (nv * 15 + nf * 12) + shape["new_v"] * 15 + shape["new_f"] * 12}
    hist = shape["hist"]
    sizes = ", ".join(f"{lo}-{hi}: {int(hist[lo:hi + 1].sum())}" for lo, hi in ((3, 3), (4, 8), (9, 16), (17, 32), (33, 64)) if lo <= args.max_edges)
    lines = [f"## One scan: the mesh of {args.views} views of {args.w}x{args.h} at voxel {args.voxel}, {6 * args.holes} places punched\n",
             f"{nv} vertices and {nf} faces ({removed} faces punched out); {shape['border']} border half-edges, {shape['regular']} regular "
             f"vertices, {shape['rounds']} doubling rounds, {shape['candidates']} candidates walked, {shape['loops']} loops filled "
             f"(edges {sizes}; the largest has {shape['largest']}), {shape['new_v']} vertices and {shape['new_f']} faces added.  "
             f"`fill_holes(max_edges={args.max_edges})`: {info}\n",
             f"Device copy of 1 GiB, measured in this run: {rate / 1e12:.2f} TB/s (read plus written).\n",
             "| phase | median ms | min | max | GB it cannot avoid | ms at the copy rate | fraction of the copy rate |\n|---|---|---|---|---|---|---|"]
    for k in PHASES:
        med = float(np.median(t[k]))
        label = {"sort": "sort (torch.sort of 3 F int64 keys)", "init": "init (rule 3, the border count's read, torch.nonzero)",
                 "doubling": f"doubling, {shape['rounds']} rounds, both directions", "offsets": "offsets (prefix sums, the ONE read)",
                 "emit": "emit (copies of the input's rows, emit kernel)"}.get(k, k)
        if k in nbytes:
            floor = nbytes[k] / rate * 1e3
            lines.append(f"| {label} | {stats(t[k])} | {nbytes[k] / 1e9:.3f} | {floor:.3f} | {floor / med if med > 0 else 0.0:.2f} |")
        else:
            lines.append(f"| {label} | {stats(t[k])} | | | |")
    total = sum(float(np.median(t[k])) for k in PHASES)
    worst = max(PHASES, key=lambda k: float(np.median(t[k])))
    lines += [f"| sum of the phases | {total:.3f} | | | | | |", f"| fill_holes, host clock | {stats(t['fill_holes'])} | | | |\n",
              f"The phase that binds is `{worst}`: {float(np.median(t[worst])):.3f} ms of {total:.3f} ms "
              f"({100.0 * float(np.median(t[worst])) / total:.0f} %).\n"]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Hole filling of a scan's mesh on the MI355X (`csrc/mesh_fill.hip`)\n\n"
                    f"`python scripts/time_mesh_fill.py --views {args.views} --h {args.h} --w {args.w} --voxel {args.voxel} --holes {args.holes} "
                    f"--max_edges {args.max_edges} --rounds {args.rounds}`, {time.strftime('%Y-%m-%d')}: {args.rounds} repetitions after a "
                    "warm-up, one process, one MI355X.  Phases between HIP events with a synchronise after each, fill_holes by the host "
                    "clock around a device synchronise.  No threshold: nothing before this does the step.  Recorded values.\n\n" + text +
                    "\n## Reading the table\n\n"
                    "- `keys` is one thread per face: 12 bytes read, three 8-byte keys written.  `border` reads every sorted key once "
                    "and its two neighbours from cache; it writes only at border half-edges.\n"
                    "- `sort` is torch's radix sort of the 3 F keys and no kernel of this library; it is reported as such, as the "
                    "cells' sort of the simplification is.\n"
                    "- `init` writes the two (label, jump) pairs of both directions for every vertex and holds the read of the border "
                    "count, which ends the work for a closed mesh, and torch.nonzero's.\n"
                    "- `doubling`, `walk` and the emit kernel run over the regular vertices only; the walk is serial per candidate, "
                    "at most max_edges steps each, and the doubling in both directions leaves at most one candidate per window of a "
                    "long rim.\n"
                    "- `emit` is the three device copies of the input's rows into the output, which dominate it, and the emit kernel.\n"
                    "\n## Not measured\n\n"
                    "- 32-bit keys for meshes of fewer than 2^15.5 vertices, or a sort of (key, slot) pairs that would let the border "
                    "kernel skip the decode.\n"
                    "- The border edges found by the counting build of the smoothing's adjacency instead of a sort.\n"
                    "- A walk spread over the lanes of a wave for rims near max_edges = 4096.\n")
        print(f"wrote {args.write}", flush=True)


if __name__ == "__main__":
    main()
