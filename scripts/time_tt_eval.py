"""Phase times of the Tanks and Temples evaluation on a synthetic scene at real size (cds_mvsnet_amd.tt_eval.evaluate): both
clouds around 20 M points at the Truck threshold tau = 0.005, the prediction with noise, holes, outliers and a small similarity
misalignment.

    python scripts/time_tt_eval.py [--repeats 2] [--n 20000000] [--tau 0.005]

Device events on the current stream bracket each phase (registration, transform, crop, voxel down-sample, pred->gt, gt->pred,
scores); the first run is a warm-up.  Prints one line per run, the ICP iterations of each registration round with the time per
iteration, and the per-phase median."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cds_mvsnet_amd import synth, tt_eval  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--n", type=int, default=20_000_000, help="points of each cloud before the holes")
    ap.add_argument("--tau", type=float, default=tt_eval.TAU["Truck"])
    args = ap.parse_args()
    t0 = time.time()
    sc = synth.make_tt_scene(n_gt=args.n, n_pred=args.n, tau=args.tau, hole_radius=150.0, seed=21)
    print(f"scene: {len(sc['pred'])} predicted, {len(sc['gt'])} ground-truth points, tau {args.tau:g} "
          f"(generated in {time.time() - t0:.1f} s)", flush=True)
    pred, gt = torch.from_numpy(sc["pred"]).cuda(), torch.from_numpy(sc["gt"]).cuda()
    runs = []
    for k in range(args.repeats + 1):
        timings = {}
        torch.cuda.synchronize()
        t1 = time.time()
        r = tt_eval.evaluate(pred, gt, sc["crop"], sc["trans"], args.tau, timings=timings)
        torch.cuda.synchronize()
        wall = (time.time() - t1) * 1e3
        if k == 0:
            print(f"cropped {r['n_pred_cropped']} / {r['n_gt_cropped']}, sampled {r['n_pred_sampled']} / {r['n_gt_sampled']}; "
                  f"precision {r['precision']:.5f} recall {r['recall']:.5f} f-score {r['fscore']:.5f}")
        dev_total = sum(timings.values())
        label = "warm-up" if k == 0 else f"run {k}"
        print(f"{label}: " + ", ".join(f"{n} {v:.1f}" for n, v in timings.items()) + f" | device {dev_total:.1f} ms, wall {wall:.1f} ms",
              flush=True)
        for i, rd in enumerate(r["registration"]):
            # a round evaluates the pair sums once more than it iterates; its time also holds the crop, the down-sampling and the grid
            print(f"  {label} round {i + 1}: {rd['n_source']} -> {rd['n_target']} points, cap {rd['cap']:g}, {rd['iterations']} iterations, "
                  f"fitness {rd['fitness']:.4f}, rmse {rd['rmse']:.3e}, {rd['ms']:.1f} ms, icp {rd['icp_ms']:.1f} ms = "
                  f"{rd['icp_ms'] / (rd['iterations'] + 1):.2f} ms per evaluation", flush=True)
        if k:
            runs.append(dict(timings, total=dev_total, wall=wall))
    if runs:
        print("median (ms): " + ", ".join(f"{n} {np.median([r[n] for r in runs]):.1f}" for n in runs[0]))


if __name__ == "__main__":
    main()
