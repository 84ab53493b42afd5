"""Phase times of the DTU evaluation on a DTU-scale synthetic scan (cds_mvsnet_amd.dtu_eval.evaluate): ~2.5 M STL points at
0.2 mm, ~25 M predicted points with noise, holes and outliers, scored at the protocol's dst 0.2 mm / max_dist 20 mm.

    python scripts/time_dtu_eval.py [--repeats 3] [--n-pred 26000000]

Device events on the current stream bracket each phase (upload, thinning, masks, grid build, data->stl, stl->data,
statistics); the first run is a warm-up.  Prints one line per run and the per-phase median."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cds_mvsnet_amd import dtu_eval, pointcloud, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-pred", type=int, default=26_000_000)
    args = ap.parse_args()
    t0 = time.time()
    sc = synth.make_dtu_scene(158, 158, 0.2, 2.0, 10.0, n_pred=args.n_pred, noise=0.12, outlier_frac=0.01, outlier_range=25.0,
                              holes=6, hole_radius=8.0, seed=21)
    print(f"scene: {len(sc['pred'])} predicted, {len(sc['stl'])} STL points, ObsMask {sc['ObsMask'].shape} "
          f"(generated in {time.time() - t0:.1f} s)", flush=True)
    pred = torch.from_numpy(sc["pred"]).cuda()
    runs = []
    for k in range(args.repeats + 1):
        timings = {}
        info = {}
        torch.cuda.synchronize()
        t1 = time.time()
        r = dtu_eval.evaluate(pred, sc, timings=timings)
        torch.cuda.synchronize()
        wall = (time.time() - t1) * 1e3
        # the thinning rounds of the same order, for the record
        if k == 0:
            pointcloud.reduce_points(pred, 0.2, seed=0, info=info)
            print(f"thinning rounds: {info['rounds']}; thinned {r['n_thinned']}, in mask {r['n_in_mask']}, "
                  f"above plane {r['n_above_plane']}; acc {r['acc']:.5f} comp {r['comp']:.5f} overall {r['overall']:.5f}")
        dev_total = sum(timings.values())
        print(f"{'warm-up' if k == 0 else f'run {k}'}: " + ", ".join(f"{n} {v:.1f}" for n, v in timings.items())
              + f" | device {dev_total:.1f} ms, wall {wall:.1f} ms", flush=True)
        if k:
            runs.append(dict(timings, total=dev_total, wall=wall))
    if runs:
        print("median (ms): " + ", ".join(f"{n} {np.median([r[n] for r in runs]):.1f}" for n in runs[0]))


if __name__ == "__main__":
    main()
