"""Time the gipuma-style fusion (cds_mvsnet_amd.gipuma) on a DTU-shaped or a Tanks & Temples-shaped synthetic scan.

    python scripts/time_gipuma.py --shape dtu [--repeats 3] [--files]
    python scripts/time_gipuma.py --shape tt  [--repeats 3] [--files]

dtu: 49 views at 1152x1536 with dtu_eval.sh's thresholds (disp 0.1, 2 consistent views, probabilities 0);
tt: 150 views at 1056x1920 with a T&T recipe's (probabilities 0.8, disp 0.3, 5 consistent views).
The scan is the height field of synth.make_fusion_scene seen by synth.make_cameras (pixel_offset 0, 15 % outliers of
+-2..6 %, confidences uniform in (0.75, 1]), rendered on the GPU in float64 (the numpy renderer would take minutes at
this size).  Per run: the device time of fuse_views (events on the current stream around the whole call) and its wall
time; the first run is a warm-up.  With --files the scan is also written in the infer layout to a temporary folder and
filter_scan is timed from the files to the PLY (PFM / JPEG reading included).  Prints (pixel, other view) pairs per
second for the nominal V h w (V - 1) pairs and, from a diagnostic pass, for the pairs the fusion kernel evaluates."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cds_mvsnet_amd import gipuma, mvs_io, synth  # noqa: E402

SHAPES = {"dtu": (49, 1152, 1536, (0.0, 0.0, 0.0), 0.1, 2), "tt": (150, 1056, 1920, (0.8, 0.8, 0.8), 0.3, 5)}


def render(V, h, w, seed=0, outlier_frac=0.15):
    """synth.make_fusion_scene's scene (pixel_offset 0) on the GPU: depths [V,h,w], confs [V,3,h,w], cams, images uint8."""
    cams = synth.make_cameras(V, h, w, refine=False, seed=seed)["stage3"][0].clone()
    cams[:, 1, 3, 3] = 1.0
    g = torch.Generator(device="cuda").manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float64),
                            torch.arange(w, device="cuda", dtype=torch.float64), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)]).reshape(3, -1)
    depths = torch.empty((V, h, w), dtype=torch.float32, device="cuda")
    for i in range(V):
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
        depths[i] = torch.where(bad, dep * (1.0 + sign * mag), dep).float()
    confs = 1.0 - 0.25 * torch.rand((V, 3, h, w), generator=g, device="cuda")     # above 0.8 in all three stages: 51 %
    images = torch.randint(0, 256, (V, h, w, 3), generator=g, device="cuda", dtype=torch.uint8)
    return depths, confs, cams, images


def phases(depths, confs, cams, images, prob, disp, ncons):
    """fuse_views' steps one by one with events between them (diagnostic pass, not timed as a whole) and the number of
    pixels that start a point search (D' in range and not used when their view's turn comes): started x (V - 1) is the
    number of (pixel, view) pairs the fusion kernel evaluates."""
    from cds_mvsnet_amd import ops
    V, h, w = depths.shape
    views, fb = gipuma.camera_constants(cams.numpy())
    views, fb = torch.from_numpy(views).cuda(), torch.from_numpy(fb).cuda()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ev[0].record()
    filt, rgb = ops.gipuma_prob_filter(depths, confs, images, prob)
    ev[1].record()
    tiles = ops.gipuma_tiles(V * h * w)
    used = torch.zeros((V, h, w), dtype=torch.uint8, device="cuda")
    emit = torch.zeros(tiles * 4096, dtype=torch.uint8, device="cuda")
    records = torch.empty((V, h, w, 4), dtype=torch.int32, device="cuda")
    valid = (filt > gipuma.DEPTH_MIN) & (filt < gipuma.DEPTH_MAX)
    started = torch.zeros((), dtype=torch.int64, device="cuda")
    waves = torch.zeros((), dtype=torch.int64, device="cuda")       # waves (64 consecutive pixels) with a started lane
    pad = (-h * w) % 64
    for r in range(V):
        st = (valid[r] & (used[r] == 0)).reshape(-1)
        started += st.sum()
        waves += torch.nn.functional.pad(st, (0, pad)).view(-1, 64).any(1).sum()
        ops.gipuma_fuse_view(r, filt, rgb, views, fb, gipuma.DEPTH_MIN, gipuma.DEPTH_MAX, disp, ncons, used, emit, records)
    ev[2].record()
    off, total = ops.gipuma_scan(emit)
    ev[3].record()
    n = int(total.item())
    ops.gipuma_compact(emit, records, off, n)
    ev[4].record()
    torch.cuda.synchronize()
    names = ("prob filter", "fusion (with the started-pixel counts)", "scan", "compaction")
    print("phases (ms): " + ", ".join(f"{k} {ev[i].elapsed_time(ev[i + 1]):.2f}" for i, k in enumerate(names)))
    st, wv = int(started), int(waves)
    print(f"pixels that start a search: {st} of {V * h * w} ({st / (V * h * w):.3f}); evaluated pairs {st * (V - 1):.3e}; "
          f"valid pixels {int(valid.sum())}; points {n}; waves with a started lane {wv} of {V * ((h * w + 63) // 64)} "
          f"(lanes busy in them {st / (64 * max(wv, 1)):.3f})", flush=True)
    return st * (V - 1)


def write_scan(folder, depths, confs, cams, images):
    from PIL import Image
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(os.path.join(folder, sub))
    for i in range(depths.shape[0]):
        mvs_io.write_pfm(os.path.join(folder, "depth_est", f"{i:08d}.pfm"), depths[i].cpu().numpy())
        mvs_io.write_pfm(os.path.join(folder, "confidence", f"{i:08d}.pfm"),
                         np.ascontiguousarray(confs[i].permute(1, 2, 0).cpu().numpy()))
        mvs_io.write_cam_file(os.path.join(folder, "cams", f"{i:08d}_cam.txt"), cams[i].numpy())
        Image.fromarray(images[i].cpu().numpy()).save(os.path.join(folder, "images", f"{i:08d}.jpg"), quality=95)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="dtu")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--files", action="store_true", help="also time filter_scan from files written in the infer layout")
    args = ap.parse_args()
    V, h, w, prob, disp, ncons = SHAPES[args.shape]
    pairs = V * h * w * (V - 1)
    t0 = time.time()
    depths, confs, cams, images = render(V, h, w)
    torch.cuda.synchronize()
    print(f"{args.shape}: {V} views at {h}x{w}, prob {prob}, disp {disp}, num_consistent {ncons}; {pairs:.3e} nominal "
          f"(pixel, view) pairs; rendered in {time.time() - t0:.1f} s", flush=True)
    dev_ms = []
    for k in range(args.repeats + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t1 = time.time()
        start.record()
        out = gipuma.fuse_views(depths, confs, cams, images, prob, disp, ncons)
        end.record()
        torch.cuda.synchronize()
        wall = (time.time() - t1) * 1e3
        d = start.elapsed_time(end)
        n = out["points"].shape[0]
        print(f"{'warm-up' if k == 0 else f'run {k}'}: device {d:.1f} ms, wall {wall:.1f} ms, {n} points "
              f"({n / (V * h * w):.3f} per pixel), {pairs / d * 1e3:.3e} pairs/s", flush=True)
        if k:
            dev_ms.append(d)
        del out
    if dev_ms:
        print(f"median device {np.median(dev_ms):.1f} ms = {pairs / np.median(dev_ms) * 1e3:.3e} pairs/s", flush=True)
        evaluated = phases(depths, confs, cams, images, prob, disp, ncons)
        print(f"evaluated pairs per second of the median run: {evaluated / np.median(dev_ms) * 1e3:.3e}", flush=True)
    if args.files:
        tmp = tempfile.mkdtemp(prefix="gipuma_time_")
        try:
            t2 = time.time()
            scan = os.path.join(tmp, "scan1")
            write_scan(scan, depths, confs, cams, images)
            print(f"wrote the scan in {time.time() - t2:.1f} s", flush=True)
            for k in range(2):
                torch.cuda.synchronize()
                t3 = time.time()
                info = gipuma.filter_scan(scan, os.path.join(tmp, "scan1.ply"), prob, disp, ncons)
                torch.cuda.synchronize()
                print(f"filter_scan {'warm-up' if k == 0 else 'run'}: wall {(time.time() - t3) * 1e3:.0f} ms from the files "
                      f"to the PLY, {info['points']} points", flush=True)
        finally:
            shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
