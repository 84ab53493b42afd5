"""Time the component kernels of csrc/mesh_clean.hip on a DTU-shaped scan: the mesh of scripts/time_tsdf_mesh.py with debris.

    python scripts/time_mesh_clean.py [--views 49 --h 864 --w 1152 --voxel 0.35] [--pieces 4000] [--min_faces 100] [--rounds 5]
        [--write profiles/mesh_components.md]

The scan and its mesh: time_tsdf_mesh.render (the height field of synth.make_fusion_scene from --views cameras), fused and
extracted by mesh.TsdfVolume at --voxel.  --pieces tetrahedra (4 vertices, 4 faces, closed) are then put into it at seeded random
places of the vertex order and of the face order, each piece's rows together, as the extractor's block order would leave debris:
not behind the surface's rows.  Before anything is timed, clean_mesh at --min_faces must return the scan's own mesh bit for bit.

Reported, each a median with minimum and maximum over --rounds after a warm-up, one process:
  init / hook / jump / count / mark / gather   the launches of mesh.clean_mesh between HIP events, through the C entry points in
                                                its order; hook and jump summed over the rounds of one labelling, and per round
  select / offsets                              the torch steps between them: the component list and rule 4; the two cumsums
  clean_mesh                                    the whole call by the host clock around a device synchronise
With each kernel the bytes it cannot avoid, computed from the shapes (below), and the fraction of the 6.3 TB/s a streaming kernel
reaches on the MI355X that they are of its time.  A walk along parent is counted as one 4-byte read per vertex of a face although
it may take more steps, and the atomics are not counted.  Recorded values, not thresholds.  There is no CPU fallback: without a
GPU the script fails."""
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

KERNELS = ("init", "hook", "jump", "count", "select", "mark", "offsets", "gather")
TETRA = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]


def add_debris(m, pieces, seed=0):
    """The mesh with `pieces` tetrahedra put in at seeded places of the vertex and the face order."""
    dev = m["vertices"].device
    nv, nf = m["vertices"].shape[0], m["faces"].shape[0]
    g = torch.Generator(device="cpu").manual_seed(seed)
    pv = torch.sort(torch.randint(0, nv + 1, (pieces,), generator=g)).values.to(dev)       # piece j stands before vertex pv[j]
    pf = torch.sort(torch.randint(0, nf + 1, (pieces,), generator=g)).values.to(dev)
    j4 = 4 * torch.arange(pieces, device=dev)
    vmap = torch.arange(nv, device=dev) + 4 * torch.searchsorted(pv, torch.arange(nv, device=dev), right=True)
    fmap = torch.arange(nf, device=dev) + 4 * torch.searchsorted(pf, torch.arange(nf, device=dev), right=True)
    vnew = (pv + j4)[:, None] + torch.arange(4, device=dev)[None]                           # [pieces, 4] rows of the pieces
    fnew = (pf + j4)[:, None] + torch.arange(4, device=dev)[None]
    lo, hi = m["vertices"].amin(0), m["vertices"].amax(0)
    centre = lo + (hi - lo) * torch.rand((pieces, 3), generator=g).to(dev)
    corner = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32, device=dev)
    vert = torch.empty((nv + 4 * pieces, 3), dtype=torch.float32, device=dev)
    col = torch.full((nv + 4 * pieces, 3), 128, dtype=torch.uint8, device=dev)
    faces = torch.empty((nf + 4 * pieces, 3), dtype=torch.int32, device=dev)
    vert[vmap], col[vmap] = m["vertices"], m["colors"]
    vert[vnew.reshape(-1)] = (centre[:, None, :] + corner[None]).reshape(-1, 3)
    faces[fmap] = vmap[m["faces"].long()].to(torch.int32)
    faces[fnew.reshape(-1)] = (vnew[:, torch.tensor(TETRA, device=dev)].reshape(-1, 3)).to(torch.int32)
    return {"vertices": vert, "colors": col, "faces": faces}


def timed_clean(lib, m, min_faces, keep_largest):
    """clean_mesh's steps with an event between them -> ({step: ms}, [ms per hook], [ms per jump], counts for the byte model)."""
    vert, col, faces = m["vertices"], m["colors"], m["faces"]
    nv, nf, dev = vert.shape[0], faces.shape[0], vert.device
    stream = torch.cuda.current_stream().cuda_stream
    parent = torch.empty(nv, dtype=torch.int32, device=dev)
    count = torch.zeros(nv, dtype=torch.int32, device=dev)
    changed = torch.zeros(mesh.MAX_ROUNDS, dtype=torch.int32, device=dev)
    ms = dict.fromkeys(KERNELS, 0.0)

    def span(name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b)
        ms[name] += t
        return out, t

    span("init", lambda: _lib.check(lib.cds_mesh_cc_init(parent.data_ptr(), nv, stream), "init"))
    hooks, jumps, rounds = [], [], 0
    while True:
        if rounds == mesh.MAX_ROUNDS:
            raise SystemExit("the labelling did not settle")
        hooks.append(span("hook", lambda: _lib.check(lib.cds_mesh_cc_hook(faces.data_ptr(), nf, nv, parent.data_ptr(),
                                                                          changed.data_ptr() + 4 * rounds, stream), "hook"))[1])
        jumps.append(span("jump", lambda: _lib.check(lib.cds_mesh_cc_jump(parent.data_ptr(), nv, stream), "jump"))[1])
        rounds += 1
        if int(changed[rounds - 1]) == 0:
            break
    span("count", lambda: _lib.check(lib.cds_mesh_cc_count(faces.data_ptr(), nf, nv, parent.data_ptr(), count.data_ptr(), stream),
                                     "count"))

    def select():
        comps = torch.nonzero(parent == torch.arange(nv, dtype=torch.int32, device=dev)).reshape(-1)
        keep = torch.zeros(nv, dtype=torch.uint8, device=dev)
        keep[comps] = mesh.select_components(count[comps], min_faces, keep_largest).to(torch.uint8)
        return comps, keep
    (comps, keep), _ = span("select", select)
    fkeep = torch.empty(nf, dtype=torch.uint8, device=dev)
    vkeep = torch.zeros(nv, dtype=torch.uint8, device=dev)
    span("mark", lambda: _lib.check(lib.cds_mesh_cc_mark(faces.data_ptr(), nf, nv, parent.data_ptr(), keep.data_ptr(),
                                                         fkeep.data_ptr(), vkeep.data_ptr(), stream), "mark"))

    def offsets():
        vend, fend = torch.cumsum(vkeep, 0, dtype=torch.int64), torch.cumsum(fkeep, 0, dtype=torch.int64)
        return (vend - vkeep).to(torch.int32), (fend - fkeep).to(torch.int32), int(vend[-1]), int(fend[-1])
    (vnew, fnew, nv_out, nf_out), _ = span("offsets", offsets)
    out = {"vertices": torch.empty((nv_out, 3), dtype=torch.float32, device=dev),
           "colors": torch.empty((nv_out, 3), dtype=torch.uint8, device=dev),
           "faces": torch.empty((nf_out, 3), dtype=torch.int32, device=dev)}
    span("gather", lambda: _lib.check(lib.cds_mesh_cc_gather(vert.data_ptr(), col.data_ptr(), faces.data_ptr(), nv, nf, vkeep.data_ptr(),
                                                             vnew.data_ptr(), fkeep.data_ptr(), fnew.data_ptr(), nv_out, nf_out,
                                                             out["vertices"].data_ptr(), out["colors"].data_ptr(),
                                                             out["faces"].data_ptr(), stream), "gather"))
    return ms, hooks, jumps, {"rounds": rounds, "components": int(comps.numel()), "nv_out": nv_out, "nf_out": nf_out}, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--h", type=int, default=864)
    ap.add_argument("--w", type=int, default=1152)
    ap.add_argument("--voxel", type=float, default=0.35)
    ap.add_argument("--pieces", type=int, default=4000)
    ap.add_argument("--min_faces", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--write", default=None, help="markdown file to record the result in")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_clean.py needs the GPU: nothing is measured without one")
    depths, masks, images, cams, points = make_scan(args.views, args.h, args.w)
    vol = mesh.TsdfVolume(points, args.voxel)
    vol.integrate(depths, masks.to(torch.uint8), images, cams)
    scan = vol.extract(2)
    del vol, points, images, depths, masks
    torch.cuda.empty_cache()
    own = mesh.mesh_components(scan["faces"], scan["vertices"].shape[0])
    own_sizes = torch.sort(own["faces"], descending=True).values
    own_unused = int((own["faces"] == 0).sum())
    print(f"scan: {scan['vertices'].shape[0]} vertices, {scan['faces'].shape[0]} faces, {own['components'].numel()} components "
          f"({own_unused} vertices in no face), the largest {own_sizes[:5].tolist()}, {own['rounds']} rounds", flush=True)
    m = add_debris(scan, args.pieces)
    nv, nf = int(m["vertices"].shape[0]), int(m["faces"].shape[0])
    print(f"with debris: {nv} vertices, {nf} faces", flush=True)

    # the check: cleaning at --min_faces gives what cleaning the scan's own mesh gives, bit for bit
    got, info = mesh.clean_mesh(m, args.min_faces)
    want, winfo = mesh.clean_mesh(scan, args.min_faces)
    for k in ("colors", "faces"):
        if not torch.equal(got[k], want[k]):
            raise SystemExit(f"the cleaned mesh differs from the scan's own in {k}")
    if not torch.equal(got["vertices"].view(torch.int32), want["vertices"].view(torch.int32)):
        raise SystemExit("the cleaned mesh differs from the scan's own in vertices")
    print(f"clean_mesh(min_faces={args.min_faces}): {info}", flush=True)
    del got, want, scan

    lib = _lib.load()
    timed_clean(lib, m, args.min_faces, 0)                                 # warm-up
    t = {k: [] for k in KERNELS + ("clean_mesh",)}
    per_hook, per_jump, shape = [], [], None
    for _ in range(args.rounds):
        ms, hooks, jumps, shape, _ = timed_clean(lib, m, args.min_faces, 0)
        for k in KERNELS:
            t[k].append(ms[k])
        per_hook.append(hooks)
        per_jump.append(jumps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh.clean_mesh(m, args.min_faces)
        torch.cuda.synchronize()
        t["clean_mesh"].append((time.perf_counter() - t0) * 1e3)

    r, vo, fo = shape["rounds"], shape["nv_out"], shape["nf_out"]
    nbytes = {"init": nv * 4,
              "hook": r * nf * (12 + 12),                                  # per round: indices, one parent word per corner
              "jump": r * nv * (4 + 4),                                    # per round: the vertex's word and its root's
              "count": nf * (12 + 4),                                      # indices, the label of the first
              "select": nv * (4 + 1),                                      # the roots found, the keep byte per vertex written
              "mark": nf * (12 + 4 + 1 + 1),                               # indices, label, keep byte, the face flag
              "offsets": (nv + nf) * (1 + 8 + 4),                          # flags in, int64 sums, int32 offsets out
              "gather": nv * (1 + 4) + vo * 2 * 15 + nf * (1 + 4) + fo * (12 + 12 + 12)}
    lines = [f"## One scan: the mesh of {args.views} views of {args.w}x{args.h} at voxel {args.voxel}, with {args.pieces} tetrahedra put in\n",
             f"{nv} vertices and {nf} faces in {shape['components']} components (the scan's own mesh: {own['components'].numel()}, of "
             f"which {own_unused} are vertices in no face; its largest have {own_sizes[:5].tolist()} faces).  min_faces = "
             f"{args.min_faces} keeps {vo} vertices and {fo} faces, bit for bit what it keeps of the scan's own mesh.  The labels "
             f"settle in {r} rounds (the last one finds nothing to lower).\n",
             "| step | median ms | min | max | GB it cannot avoid | fraction of 6.3 TB/s |\n|---|---|---|---|---|---|"]
    for k in KERNELS:
        med = float(np.median(t[k]))
        floor = nbytes[k] / (STREAM_TBS * 1e12) * 1e3
        lines.append(f"| {k} | {stats(t[k])} | {nbytes[k] / 1e9:.3f} | {floor / med if med > 0 else 0.0:.2f} |")
    lines.append(f"| sum of the steps | {sum(float(np.median(t[k])) for k in KERNELS):.3f} | | | | |")
    lines.append(f"| clean_mesh, host clock | {stats(t['clean_mesh'])} | | |\n")
    lines += ["### Per round, ms (median over the repetitions)\n", "| round | hook | jump | compulsory GB (hook + jump) |\n|---|---|---|---|"]
    for i in range(r):
        lines.append(f"| {i + 1} | {np.median([h[i] for h in per_hook]):.3f} | {np.median([j[i] for j in per_jump]):.3f} | "
                     f"{(nf * 24 + nv * 8) / 1e9:.3f} |")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Connected components and clean-up of a scan's mesh on the MI355X (`csrc/mesh_clean.hip`)\n\n"
                    f"`python scripts/time_mesh_clean.py --views {args.views} --h {args.h} --w {args.w} --voxel {args.voxel} --pieces "
                    f"{args.pieces} --min_faces {args.min_faces} --rounds {args.rounds}`: {args.rounds} repetitions after a warm-up, one "
                    "process, one MI355X.  Kernels between HIP events with a synchronise after each (as the host loop has after every "
                    "hook), clean_mesh by the host clock around a device synchronise.  Recorded values, not thresholds.\n\n" + text +
                    "\n\n## Measured once, on this scan, while count was written\n\n"
                    "- count with one wave per 64 faces, that is one add to the surface's counter per wave, 656 k adds to one "
                    "address: 7.448 ms, the slowest step of a 16.8 ms clean_mesh.  A wave now takes 16 runs of 64 faces and holds "
                    "the sum of the first label it meets in a register: the figure in the table.\n"
                    "\n## Not measured\n\n"
                    "- count without any aggregation inside the wave (one atomicAdd per face), and a sum across the four waves of "
                    "a workgroup through LDS.\n"
                    "- A single-kernel union-find with compare-and-swap hooking and no host loop, against this round-based form "
                    "and its one word read per round.\n"
                    "- Plain loads in jump (its reads are of words that other workgroups of the same launch replace by "
                    "ancestors, so they would be correct); the agent-scope atomic loads were kept there for one find routine.\n"
                    "- Hook rounds that skip the faces whose vertices already shared a root in the round before.\n")
        print(f"wrote {args.write}", flush=True)


if __name__ == "__main__":
    main()
