"""Time the COLMAP -> MVSNet conversion on synthetic models (records for profiles/colmap_convert.md, not thresholds).

    python scripts/time_colmap.py [--sizes 300x200000,1000x1000000] [--ref] [--json out.json]

Per size (images x points, mean track length ~6, ``synth.make_colmap_model``): device time of the pair-score kernel and of
the depth-range step (two kernels and the torch sort between them), wall time of a whole ``colmap.convert`` from a binary
model on disk, and with ``--ref`` the wall time of the float64 numpy restatement ``tests/colmap_ref.py`` on 16 threads."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cds_mvsnet_amd import colmap, ops, synth  # noqa: E402

ATOMIC_RATE = 1.3e12     # bytes / s: the chip-wide rate of well-shaped global float atomic adds on the MI355X, for comparison


def _device_ms(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def run(n_images, n_points, with_ref, long_frac):
    t0 = time.time()
    model = synth.make_colmap_model(n_images, n_points, seed=n_images, long_frac=long_frac, min_angle_deg=None)
    rec = {"images": n_images, "points": n_points, "generate_s": round(time.time() - t0, 2),
           "mean_track": float(np.diff(model[2].track_ptr).mean()), "max_track": int(np.diff(model[2].track_ptr).max())}
    tmp = tempfile.mkdtemp()
    try:
        dense = os.path.join(tmp, "dense")
        colmap.write_model(os.path.join(dense, "sparse"), ".bin", *model)
        os.makedirs(os.path.join(dense, "images"))
        from PIL import Image
        for im in model[1].values():
            Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(os.path.join(dense, "images", im.name))
        t0 = time.time()
        out = colmap.convert(dense, os.path.join(tmp, "scene"))
        rec["convert_wall_s"] = round(time.time() - t0, 3)
        t0 = time.time()
        cameras, images, points = colmap.read_model(os.path.join(dense, "sparse"), ".bin")
        rec["read_model_s"] = round(time.time() - t0, 3)
    finally:
        shutil.rmtree(tmp)
    ext, _, centres = colmap.scene_cameras(cameras, images)
    obs_img, obs_pt, xyz, counts = colmap._device_observations(images, points, "cuda")
    N, P = len(images), len(points)
    csr = ops.colmap_point_csr(obs_img, obs_pt, N, P)
    ctr = torch.from_numpy(centres).cuda()
    rec["observations"], rec["terms"] = int(obs_img.numel()), int(csr[4])
    rec["pair_scores_kernel_ms"] = round(_device_ms(lambda: ops.colmap_pair_scores_csr(*csr, xyz, ctr, 5.0, 1.0, 10.0)), 3)
    rec["point_csr_ms"] = round(_device_ms(lambda: ops.colmap_point_csr(obs_img, obs_pt, N, P)), 3)
    nmin, nmax = (torch.from_numpy(a).cuda() for a in colmap.range_counts(counts))
    zrow = torch.from_numpy(np.ascontiguousarray(ext[:, 2, :])).cuda()
    rec["depth_ranges_ms"] = round(_device_ms(lambda: ops.colmap_depth_ranges(obs_img, obs_pt, xyz, zrow, nmin, nmax)), 3)
    acc = ops.colmap_pair_scores_csr(*csr, xyz, ctr, 5.0, 1.0, 10.0)
    # an upper bound of the atomic traffic: two 8-byte adds per term (a limb that is zero issues none)
    rec["atomic_GBps_upper"] = round(rec["terms"] * 16 / (rec["pair_scores_kernel_ms"] * 1e-3) / 1e9, 1)
    rec["atomic_rate_fraction_upper"] = round(rec["atomic_GBps_upper"] * 1e9 / ATOMIC_RATE, 4)
    if with_ref:
        import colmap_ref as R
        t0 = time.time()
        S, n = R.pair_scores(centres, obs_img.cpu().numpy().astype(np.int64), obs_pt.cpu().numpy(), points.xyz, threads=16)
        rec["ref_pair_scores_wall_s"] = round(time.time() - t0, 2)
        t0 = time.time()
        R.depth_min_max(ext, obs_img.cpu().numpy(), obs_pt.cpu().numpy(), points.xyz)
        rec["ref_depth_ranges_wall_s"] = round(time.time() - t0, 2)
        got = ops.colmap_scores_from_limbs(acc).cpu().numpy()
        rec["max_abs_dS_per_term"] = float(np.max(np.abs(got - S) / np.maximum(n, 1)))
        assert np.array_equal(got, out["score"])
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="300x200000,1000x1000000")
    ap.add_argument("--long_frac", default="0.01,0.001", help="per size: fraction of tracks with a uniform length in [2, N]")
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    recs = []
    sizes, fracs = a.sizes.split(","), a.long_frac.split(",")
    if len(fracs) != len(sizes):
        ap.error(f"--long_frac needs one entry per size: {len(sizes)} sizes, {len(fracs)} fractions")
    for size, lf in zip(sizes, fracs):
        n, p = (int(v) for v in size.split("x"))
        recs.append(run(n, p, a.ref, float(lf)))
        print(json.dumps(recs[-1]), flush=True)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
