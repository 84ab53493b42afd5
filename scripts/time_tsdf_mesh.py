"""Time the mesher of csrc/tsdf.hip on a DTU-shaped scan: allocation, integration and extraction.

    python scripts/time_tsdf_mesh.py [--views 49 --h 864 --w 1152 --voxel 0.35] [--rounds 5] [--write profiles/tsdf_mesh.md]
        [--mesh_weight angle|conf|angle_conf] [--mesh_interp]

The scan: the height field of synth.make_fusion_scene rendered on the GPU from --views cameras of synth.make_cameras (noise-free
depth maps through the pixel centres, every pixel kept except an 8-pixel border, random images).  The kept points of all views
fix the frame and the allocated blocks, as in mesh.mesh_views.

Reported, each a median with minimum and maximum over --rounds after a warm-up, the variants alternating inside every round, one
process:
  allocation    TsdfVolume(points, voxel): keys, unique, dilation, the dense block table and the zeroed accumulators
  integration   TsdfVolume.integrate of all views with 32 views per launch (the default), 16, and 1 (the same kernel launched
                once per view: the volume is then read and written once per view), between two HIP events
  extraction    TsdfVolume.extract(2): classify, two prefix sums, emit
  weighted      with --mesh_weight / --mesh_interp: the integration of all views, 32 per launch, without weights
                (the baseline), with the weight maps of the mode, and with them and the interpolated depth, alternating inside
                every round, and the time the weight maps take (profiles/tsdf_weighted.md)
The floor of an integration is its compulsory traffic at the 6.3 TB/s a streaming kernel reaches on the MI355X: 24 B per
lattice point read and written once per launch, plus the maps (8 B per pixel) once.  Before anything is timed the volumes of
the three chunk sizes are compared: they must be equal bit for bit.  Recorded values, not thresholds.  There is no CPU
fallback: without a GPU the script fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cds_mvsnet_amd import mesh, synth  # noqa: E402

STREAM_TBS = 6.3          # what a streaming kernel reaches on the MI355X (8.0 TB/s is the HBM3E specification)
BORDER = 8


def render(n_views, h, w, seed=0):
    """depths [N,h,w], masks bool [N,h,w], images uint8 [N,h,w,3] (device), cams [N,2,4,4] (host), points [M,3] (device)."""
    cams = synth.make_cameras(n_views, h, w, refine=False, seed=seed)["stage3"][0].clone()
    cams[:, 1, 3, 3] = 1.0
    g = torch.Generator(device="cuda").manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float64) + 0.5,
                            torch.arange(w, device="cuda", dtype=torch.float64) + 0.5, indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)]).reshape(3, -1)
    depths = torch.empty((n_views, h, w), dtype=torch.float32, device="cuda")
    masks = torch.zeros((n_views, h, w), dtype=torch.bool, device="cuda")
    masks[:, BORDER:h - BORDER, BORDER:w - BORDER] = True
    points = []
    for i in range(n_views):
        E, K = cams[i, 0].double().cuda(), cams[i, 1, :3, :3].double().cuda()
        R, t = E[:3, :3], E[:3, 3:4]
        rd, rt = R.T @ (torch.linalg.inv(K) @ pix), R.T @ t
        lam = torch.full((pix.shape[1],), 650.0, dtype=torch.float64, device="cuda")
        for _ in range(20):
            P = rd * lam - rt
            lam = (650.0 + 40.0 * torch.sin(P[0] / 60.0) * torch.cos(P[1] / 50.0) + rt[2]) / rd[2]
        depths[i] = lam.reshape(h, w).float()
        points.append((rd * depths[i].reshape(-1).double() - rt).t()[masks[i].reshape(-1)].float())
    images = torch.randint(0, 256, (n_views, h, w, 3), generator=g, device="cuda", dtype=torch.uint8)
    return depths, masks, images, cams, torch.cat(points).contiguous()


def stats(v):
    return f"{np.median(v):.3f} | {min(v):.3f} | {max(v):.3f}"


def kernel_resources():
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"), "tsdf.hip"], capture_output=True,
                           text=True, timeout=300)
        return [ln.rstrip() for ln in r.stdout.splitlines() if "tsdf_" in ln] or ["not available"]
    except (OSError, subprocess.SubprocessError) as e:
        return [f"not available ({e})"]


def weighted_section(args, fresh, depths, masks8, images, cams, V):
    """The integration of all views, 32 per launch, in the modes of DESIGN §1.14, alternating inside every round with the
    unweighted kernel as the baseline; every mode adds to a volume of its own.  -> lines of the report."""
    mode = args.mesh_weight
    weights, t_maps = None, []
    if mode != "one":
        g = torch.Generator(device="cuda").manual_seed(1)
        confs = torch.rand(depths.shape, generator=g, device="cuda") if mode != "angle" else [None] * V
        for _ in range(args.rounds + 1):                          # the first is the warm-up
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            weights = torch.stack([mesh.view_weights(depths[i], masks8[i], cams[i], confs[i], mode=mode) for i in range(V)])
            end.record()
            torch.cuda.synchronize()
            t_maps.append(start.elapsed_time(end))
    modes = [("one (cds_tsdf_integrate_f32, the baseline)", {})]
    if mode != "one":
        modes.append((f"{mode}, nearest pixel", dict(weights=weights)))
    if args.mesh_interp:
        modes.append((f"{mode}, interpolated depth", dict(weights=weights, interp=True)))
    vols = [fresh() for _ in modes]
    times = [[] for _ in modes]
    for r in range(args.rounds + 1):                              # the first round is the warm-up
        for vol, (_, kw), t in zip(vols, modes, times):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            vol.integrate(depths, masks8, images, cams, **kw)
            end.record()
            torch.cuda.synchronize()
            if r:
                t.append(start.elapsed_time(end))
    lines = [f"\n## Weighted integration (DESIGN §1.14): {V} views, 32 per launch\n", "| mode | median ms | min | max | note |\n|---|---|---|---|---|"]
    base = np.median(times[0])
    for (name, _), t in zip(modes, times):
        lines.append(f"| {name} | {stats(t)} | {np.median(t) / base:.2f} x the baseline |")
    if t_maps:
        share = float((weights > 1).float().mean())
        lines.append(f"| weight maps of {V} views ({mode}: normals, then cds_tsdf_view_weights) | {stats(t_maps[1:])} | "
                     f"{100 * share:.1f} % of the pixels weigh more than 1 |")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--h", type=int, default=864)
    ap.add_argument("--w", type=int, default=1152)
    ap.add_argument("--voxel", type=float, default=0.35)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--write", default=None, help="markdown file to record the result in")
    ap.add_argument("--mesh_weight", default="one", choices=list(mesh.WEIGHT_MODES),
                    help="also time the weighted integration of DESIGN §1.14 with the weight maps of this mode")
    ap.add_argument("--mesh_interp", action="store_true", help="also time the integration with the interpolated depth")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_tsdf_mesh.py needs the GPU: nothing is measured without one")
    V, h, w = args.views, args.h, args.w
    depths, masks, images, cams, points = render(V, h, w)
    masks8 = masks.to(torch.uint8)

    def fresh():
        return mesh.TsdfVolume(points, args.voxel)

    def sync_ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    # the same volume whatever the chunk (also the warm-up of every shape)
    chunks = (32, 16, 1)
    vols = {}
    for c in chunks:
        vols[c] = fresh()
        vols[c].integrate(depths, masks8, images, cams, chunk=c)
    for c in chunks[1:]:
        for name in ("sum", "n", "nc", "rgb"):
            if not torch.equal(getattr(vols[c], name), getattr(vols[32], name)):
                raise SystemExit(f"chunk {c} and chunk 32 disagree in {name}")
    vol = vols[32]
    del vols
    blocks, pts = vol.n_blocks, vol.n_blocks * 512
    seen = float((vol.n > 0).float().mean())
    out = vol.extract(2)
    nv, nf = out["vertices"].shape[0], out["faces"].shape[0]

    t_alloc, t_int, t_ext = [], {c: [] for c in chunks}, []
    for _ in range(args.rounds):
        v2, ms = sync_ms(fresh)
        del v2
        t_alloc.append(ms)
        for c in chunks:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            vol.integrate(depths, masks8, images, cams, chunk=c)
            end.record()
            torch.cuda.synchronize()
            t_int[c].append(start.elapsed_time(end))
        t_ext.append(sync_ms(lambda: vol.extract(2))[1])

    def floor_ms(c):
        launches = (V + c - 1) // c
        return (launches * pts * 24 * 2 + V * h * w * 8) / (STREAM_TBS * 1e12) * 1e3

    lines = [f"## One scan: {V} views of {w}x{h}, voxel {args.voxel}\n",
             f"{points.shape[0]} kept points, a grid of {vol.nb[0]} x {vol.nb[1]} x {vol.nb[2]} blocks, {blocks} allocated "
             f"({pts} lattice points, {pts * 24 / 1e9:.2f} GB of accumulators), {100 * seen:.1f} % of them seen by a view; "
             f"the mesh has {nv} vertices and {nf} faces.  The volumes of 32, 16 and 1 views per launch are equal bit for bit.\n",
             "| step | median ms | min | max | note |\n|---|---|---|---|---|",
             f"| allocation (TsdfVolume) | {stats(t_alloc)} | host clock around a synchronise; sort-based unique of {points.shape[0]} keys |"]
    for c in chunks:
        f = floor_ms(c)
        lines.append(f"| integration, {c} views per launch ({(V + c - 1) // c} launches) | {stats(t_int[c])} | traffic floor {f:.3f} ms at "
                     f"{STREAM_TBS} TB/s: fraction {f / np.median(t_int[c]):.2f}; {np.median(t_int[c]) / np.median(t_int[32]):.2f} x the default |")
    lines.append(f"| extraction (classify, prefix sums, emit) | {stats(t_ext)} | host clock around a synchronise; includes one read-back "
                 "of the two totals |")
    if args.mesh_weight != "one" or args.mesh_interp:
        lines += weighted_section(args, fresh, depths, masks8, images, cams, V)
    lines.append("\n## Kernel resources (`scripts/kernel_resources.py tsdf.hip`)\n\n```\n" + "\n".join(kernel_resources()) + "\n```")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("# TSDF fusion and tetrahedra extraction on the MI355X (`csrc/tsdf.hip`)\n\n"
                    f"`scripts/time_tsdf_mesh.py`: {args.rounds} rounds after a warm-up of every variant, the variants alternating inside "
                    "each round, one process, one MI355X.  Integration between two HIP events, allocation and extraction by the host "
                    "clock around a device synchronise.  Recorded values, not thresholds.\n\n" + text + "\n")
        print(f"wrote {args.write}", flush=True)


if __name__ == "__main__":
    main()
