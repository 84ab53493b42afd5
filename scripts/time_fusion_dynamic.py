"""Time the normal and the dynamic depth-fusion kernel (ops.depth_fusion, ops.depth_fusion_dynamic) on the same inputs.

    python scripts/time_fusion_dynamic.py [--h 1088 --w 1920 --views 10] [--launches 20 --rounds 10] [--write profiles/fusion_dynamic.md]

The default is the Tanks and Temples shape: one reference view of 1920x1088 with 10 source views.  The scene is the height
field of synth.make_fusion_scene seen by synth.make_cameras (pixel centres at +0.5, 5 % outliers of +-2..6 %, every source
depth multiplied by 1 + u 12 / 1300 with u uniform in (-1, 1), so that the levels of the dynamic check spread over 1..11),
rendered on the GPU in float64; confidences are uniform in [0, 1) with thresholds (0.05, 0.03, 0.02).

Each timed window is --launches back-to-back launches of one kernel between two HIP events on the current stream; the
variants (normal, dynamic, dynamic with its optional admit / levels outputs) alternate inside every round, after a warm-up
of each, in one process.  Reported: the median and the minimum over the rounds of the time per launch, and the ratios of
the medians.  --write also records them, with the compiler's register / scratch / occupancy figures of both kernels
(scripts/kernel_resources.py), in a markdown file.  There is no CPU fallback: without a GPU the script fails."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cds_mvsnet_amd import fusion, ops, synth  # noqa: E402

CONF = (0.05, 0.03, 0.02)
AMP = 12.0


def render(n_views, h, w, seed=0, outlier_frac=0.05):
    """synth.make_fusion_scene's scene (pixel_offset 0.5) on the GPU: depths [N,h,w], confs [N,3,h,w] (device), cams (host)."""
    cams = synth.make_cameras(n_views, h, w, refine=False, seed=seed)["stage3"][0].clone()
    cams[:, 1, 3, 3] = 1.0
    g = torch.Generator(device="cuda").manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float64) + 0.5,
                            torch.arange(w, device="cuda", dtype=torch.float64) + 0.5, indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)]).reshape(3, -1)
    depths = torch.empty((n_views, h, w), dtype=torch.float32, device="cuda")
    for i in range(n_views):
        E = cams[i, 0].double().cuda()
        K = cams[i, 1, :3, :3].double().cuda()
        R, t = E[:3, :3], E[:3, 3:4]
        rd, rt = R.T @ (torch.linalg.inv(K) @ pix), R.T @ t
        lam = torch.full((pix.shape[1],), 650.0, dtype=torch.float64, device="cuda")
        for _ in range(20):
            P = rd * lam - rt
            lam = (650.0 + 40.0 * torch.sin(P[0] / 60.0) * torch.cos(P[1] / 50.0) + rt[2]) / rd[2]
        dep = lam.reshape(h, w)
        bad = torch.rand((h, w), generator=g, device="cuda", dtype=torch.float64) < outlier_frac
        sign = torch.where(torch.rand((h, w), generator=g, device="cuda") < 0.5, -1.0, 1.0).double()
        mag = 0.02 + 0.04 * torch.rand((h, w), generator=g, device="cuda", dtype=torch.float64)
        dep = torch.where(bad, dep * (1.0 + sign * mag), dep)
        if i > 0:
            u = torch.rand((h, w), generator=g, device="cuda", dtype=torch.float64) * 2.0 - 1.0
            dep = dep * (1.0 + u * (AMP / 1300.0))
        depths[i] = dep.float()
    confs = torch.rand((n_views, 3, h, w), generator=g, device="cuda")
    return depths, confs, cams


def kernel_resources():
    """The lines scripts/kernel_resources.py prints for the two kernels (a compile, no GPU work), or why there are none."""
    lines = []
    for src in ("fusion.hip", "fusion_dynamic.hip"):
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"), src], capture_output=True,
                               text=True, timeout=300)
            lines += [ln.strip() for ln in r.stdout.splitlines() if "depth_fusion" in ln]
        except (OSError, subprocess.SubprocessError) as e:
            lines.append(f"{src}: not available ({e})")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--h", type=int, default=1088)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--views", type=int, default=10, help="source views")
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--write", default=None, help="markdown file to record the result in")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_fusion_dynamic.py needs the GPU: nothing is measured without one")
    V, h, w = args.views, args.h, args.w
    depths, confs, cams = render(V + 1, h, w)
    chains = fusion.camera_chains(cams[0], cams[1:]).cuda()
    rd, rc, sd, sc = depths[0].contiguous(), confs[0].contiguous(), depths[1:].contiguous(), confs[1:].contiguous()
    variants = {
        "normal": lambda: ops.depth_fusion(rd, rc, sd, sc, chains, CONF, 1.0, 0.01, 3),
        "dynamic": lambda: ops.depth_fusion_dynamic(rd, rc, sd, sc, chains, CONF),
        "dynamic + admit + levels": lambda: ops.depth_fusion_dynamic(rd, rc, sd, sc, chains, CONF, want_admit=True,
                                                                     want_levels=True),
    }
    out_n = variants["normal"]()
    out_d = variants["dynamic + admit + levels"]()
    torch.cuda.synchronize()
    kept_n, kept_d = float(out_n[1].mean()), float(out_d[1].mean())
    hist = torch.bincount(out_d[4].reshape(-1).long(), minlength=12).cpu().numpy() / float(out_d[4].numel())
    print(f"{V} source views at {h}x{w}: normal keeps {kept_n:.3f}, dynamic keeps {kept_d:.3f}; level shares 1..11: "
          + " ".join(f"{x:.3f}" for x in hist[1:12]), flush=True)
    for f in variants.values():          # warm-up of every variant
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, f in variants.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.launches):
                f()
            end.record()
            torch.cuda.synchronize()
            ms[k].append(start.elapsed_time(end) / args.launches)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"{k:26s} median {med[k]:.4f} ms, min {min(v):.4f} ms, max {max(v):.4f} ms per launch "
              f"({args.rounds} rounds of {args.launches} launches)", flush=True)
    ratio = med["dynamic"] / med["normal"]
    ratio_all = med["dynamic + admit + levels"] / med["normal"]
    print(f"dynamic / normal = {ratio:.3f}; with admit and levels = {ratio_all:.3f}", flush=True)
    if args.write:
        res = kernel_resources()
        with open(args.write, "w") as f:
            f.write("# Dynamic-consistency fusion against the normal fusion on the MI355X (`csrc/fusion_dynamic.hip`, `csrc/fusion.hip`)\n\n")
            f.write(f"`scripts/time_fusion_dynamic.py`: one reference view of {w}x{h} with {V} source views, the height field of\n"
                    "`synth.make_fusion_scene` rendered on the GPU (5 % outliers, source depths jittered by up to 12/1300 so that\n"
                    "the levels spread), confidence thresholds (0.05, 0.03, 0.02). Both kernels read the same tensors. HIP events\n"
                    f"around {args.launches} back-to-back launches, {args.rounds} rounds, the variants alternating inside each round "
                    "after a warm-up, one process, one MI355X.\n\n")
            f.write("| kernel | median ms per launch | min | max | ratio to normal (medians) |\n|---|---|---|---|---|\n")
            for k, v in ms.items():
                f.write(f"| {k} | {med[k]:.4f} | {min(v):.4f} | {max(v):.4f} | {med[k] / med['normal']:.3f} |\n")
            f.write(f"\nThe normal rule (1 px, 1 %, 3 views) keeps {kept_n:.3f} of the pixels of this scene, the dynamic rule "
                    f"(0.25 px, 1/1300, 2..10 views) {kept_d:.3f}.\nShares of the (view, pixel) levels 1..11 (11 = inconsistent): "
                    + " ".join(f"{x:.3f}" for x in hist[1:12]) + ".\n\n")
            f.write("## Kernel resources (`scripts/kernel_resources.py`)\n\n```\n" + "\n".join(res) + "\n```\n\n")
            f.write("The dynamic kernel issues the normal kernel's loads and re-projection, then per view the level search (at most\n"
                    "n_max pairs of multiply + compare), 16 counter updates in registers and one byte store when the levels are asked\n"
                    f"for. Measured ratio {ratio:.3f} ({ratio_all:.3f} with both optional outputs)"
                    + (": within the 1.25x that would ask for an explanation.\n" if ratio <= 1.25 else
                       ": above 1.25x; compare the occupancy and scratch columns above.\n")
                    + "No scratch in either kernel (`sspill` counts scalar registers parked in vector-register lanes, not memory).\n")
        print(f"wrote {args.write}", flush=True)


if __name__ == "__main__":
    main()
