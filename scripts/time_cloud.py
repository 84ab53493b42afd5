"""Time the two kernels of csrc/cloud.hip: the normals of one depth map beside the fusion of the same view, and one voxel
merge of a scan-sized cloud.

    python scripts/time_cloud.py [--h 1184 --w 1600 --views 10] [--points 25000000 --per_voxel 10] [--launches 20 --rounds 10]
                                 [--write profiles/cloud_normals.md]

Normals: the scene of scripts/time_fusion_dynamic.py (the height field of synth.make_fusion_scene rendered on the GPU, 5 %
outliers) at the DTU full-resolution shape, one reference view with 10 source views.  ops.depth_normals (radius 1..4, with the
valid map that filter_depth passes) and the normal fusion kernel read the same reference view.  The floor of the normals kernel
is its compulsory traffic, 4 B read and 13 B written per pixel (18 B with the valid map), at the 6.3 TB/s a streaming kernel
reaches on the MI355X; the view's 32 MB fit the Infinity Cache, so back-to-back launches can beat an HBM floor and the fraction
is an orientation, not a bound.

Merge: --points uniform samples of the same height field over a square sized for --per_voxel points per voxel of side 1, random
colours and unit normals.  Timed: pointcloud.merge_voxels as a whole (keys, stable sort, unique, offsets, kernel, colour packing)
and cds_voxel_merge_f32 alone on the prepared groups.

Each timed window is --launches back-to-back calls between two HIP events (one call for the merge), the variants alternating
inside every round after a warm-up, one process.  Reported: median, minimum and maximum over the rounds.  These are recorded
values, not thresholds.  There is no CPU fallback: without a GPU the script fails."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cds_mvsnet_amd import _lib, fusion, ops, pointcloud  # noqa: E402
from cds_mvsnet_amd._lib import check  # noqa: E402
from time_fusion_dynamic import CONF, render  # noqa: E402

STREAM_TBS = 6.3          # what a streaming kernel reaches on the MI355X (8.0 TB/s is the HBM3E specification)


def timed(variants, launches, rounds):
    """name -> [ms per call] over the rounds; the variants alternate inside each round."""
    for f in variants.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(launches):
                f()
            end.record()
            torch.cuda.synchronize()
            ms[k].append(start.elapsed_time(end) / launches)
    return ms


def row(name, v, extra=""):
    return f"| {name} | {np.median(v):.4f} | {min(v):.4f} | {max(v):.4f} | {extra} |"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--h", type=int, default=1184)
    ap.add_argument("--w", type=int, default=1600)
    ap.add_argument("--views", type=int, default=10, help="source views of the fusion kernel")
    ap.add_argument("--points", type=int, default=25_000_000)
    ap.add_argument("--per_voxel", type=float, default=10.0)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--write", default=None, help="markdown file to record the result in")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_cloud.py needs the GPU: nothing is measured without one")
    V, h, w = args.views, args.h, args.w
    lines = []

    # ------------------------------------------------------------------------------------------------------- normals
    depths, confs, cams = render(V + 1, h, w)
    chains = fusion.camera_chains(cams[0], cams[1:]).cuda()
    rd, rc, sd, sc = depths[0].contiguous(), confs[0].contiguous(), depths[1:].contiguous(), confs[1:].contiguous()
    K, E = cams[0, 1, :3, :3], cams[0, 0]
    valid = (rc > torch.tensor(CONF, device="cuda").view(3, 1, 1)).all(0)
    variants = {"fusion (normal), %d source views" % V: lambda: ops.depth_fusion(rd, rc, sd, sc, chains, CONF, 1.0, 0.01, 3)}
    for r in (1, 2, 3, 4):
        variants[f"normals r={r}, valid map"] = lambda r=r: ops.depth_normals(rd, K, E, valid=valid, radius=r)
    variants["normals r=2, no valid map"] = lambda: ops.depth_normals(rd, K, E, radius=2)
    ok_share = float(ops.depth_normals(rd, K, E, valid=valid)[1].float().mean())
    ms = timed(variants, args.launches, args.rounds)
    fus = float(np.median(next(iter(ms.values()))))
    lines.append(f"## Normals of one {w}x{h} view\n")
    lines.append(f"ok share at r=2 with the valid map (confidences above {CONF}): {ok_share:.3f}.\n")
    lines.append("| kernel | median ms per launch | min | max | note |\n|---|---|---|---|---|")
    for k, v in ms.items():
        if k.startswith("normals"):
            bpp = 18 if "no valid" not in k else 17
            floor = bpp * h * w / (STREAM_TBS * 1e12) * 1e3
            extra = (f"{bpp} B/pixel floor {floor:.4f} ms at {STREAM_TBS} TB/s: fraction {floor / np.median(v):.2f}; "
                     f"{np.median(v) / fus:.3f} of the fusion kernel")
        else:
            extra = "the kernel that runs once per view beside it"
        lines.append(row(k, v, extra))

    # --------------------------------------------------------------------------------------------------------- merge
    del depths, confs, sd, sc
    n = args.points
    g = torch.Generator(device="cuda").manual_seed(1)
    side = float(np.sqrt(n / args.per_voxel))
    xy = torch.rand((n, 2), generator=g, device="cuda") * side
    z = 650.0 + 40.0 * torch.sin(xy[:, 0] / 60.0) * torch.cos(xy[:, 1] / 50.0)
    pts = torch.cat([xy, z[:, None]], 1).contiguous()
    col = torch.randint(0, 256, (n, 3), generator=g, device="cuda", dtype=torch.uint8)
    nrm = torch.nn.functional.normalize(torch.randn((n, 3), generator=g, device="cuda"), dim=1).contiguous()
    packed = pointcloud.pack_colors(col)
    perm, start, ukeys, counts = pointcloud.voxel_groups(pts, 1.0)
    v = ukeys.numel()
    out_p, out_n = torch.empty((v, 3), device="cuda"), torch.empty((v, 3), device="cuda")
    out_c, out_k = torch.empty(v, dtype=torch.int32, device="cuda"), torch.empty(v, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        check(lib.cds_voxel_merge_f32(pts.data_ptr(), packed.data_ptr(), nrm.data_ptr(), n, perm.data_ptr(), start.data_ptr(), v,
                                      out_p.data_ptr(), out_c.data_ptr(), out_n.data_ptr(), out_k.data_ptr(), stream),
              "cds_voxel_merge_f32")

    def mean_kernel():
        check(lib.cds_voxel_mean_f32(pts.data_ptr(), n, perm.data_ptr(), start.data_ptr(), v, out_p.data_ptr(), stream),
              "cds_voxel_mean_f32")

    ms2 = timed({"merge_voxels, whole (keys, sort, offsets, kernel)": lambda: pointcloud.merge_voxels(pts, col, 1.0, normals=nrm),
                 "cds_voxel_merge_f32 alone": kernel, "cds_voxel_mean_f32 alone (positions only)": mean_kernel}, 1,
                max(3, args.rounds // 2))
    lines.append(f"\n## One merge of {n} points\n")
    lines.append(f"{v} voxels of side 1, mean {n / v:.1f} points per voxel, max {int(counts.max())}, "
                 f"{float((counts == 1).float().mean()):.3f} singletons.\n")
    lines.append("| step | median ms | min | max | note |\n|---|---|---|---|---|")
    gb = (n * (8 + 12 + 4 + 12) + v * (4 + 12 + 4 + 12 + 4)) / 1e9
    for k, val in ms2.items():
        lines.append(row(k, val, f"{gb:.2f} GB of compulsory traffic (gathered through perm)" if k.startswith("cds_voxel_merge") else ""))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write("# Normals and voxel merge of fused clouds on the MI355X (`csrc/cloud.hip`)\n\n"
                    f"`scripts/time_cloud.py`: HIP events around {args.launches} back-to-back launches (one call for the merge), "
                    f"{args.rounds} rounds, the variants alternating inside each round after a warm-up, one process, one MI355X.  "
                    "Recorded values, not thresholds.  The floor is the compulsory traffic at the 6.3 TB/s of a streaming kernel; one "
                    "view fits the Infinity Cache, so a fraction above 1 means cache, not a mistake.\n\n" + text + "\n")
        print(f"wrote {args.write}", flush=True)


if __name__ == "__main__":
    main()
