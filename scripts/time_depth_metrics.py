"""Time of the twelve validation metrics of one sample (cds_mvsnet_amd.depth_eval.validation_scalars: one pass of
csrc/depth_metrics.hip + one device-to-host read) next to the same twelve metrics written in torch ops the reference's way
(tests/depth_eval_ref.torch_validation_scalars: a masked index, a compare and a mean per metric, each read back with .item()),
on the same device tensors.

    python scripts/time_depth_metrics.py [--repeats 300] [--warmup 30] [--json out.json]

Sizes: 1152 x 864 and 1600 x 1184, B = 1, a DTU-like error distribution with ~75 % of the pixels masked in.  Every call is timed on
the host from before the call to after its last host read (both formulations END in a host read, so the clock stops on finished work);
the interval tensor lives on the device as in validate().  Reported: the median and the min / max over the repeats, after the warm-up
calls, with the two formulations alternating inside the loop; the scalars of the two are compared before anything is timed."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_eval_ref as R  # noqa: E402
from cds_mvsnet_amd import depth_eval  # noqa: E402

SIZES = ((864, 1152), (1184, 1600))


def inputs(h, w, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    gt = 450.0 + 450.0 * torch.rand(1, h, w, generator=g)
    err = torch.randn(1, h, w, generator=g).abs() * 6.0                       # mm: errors from 0 to ~25, all six bands filled
    est = gt + err * torch.where(torch.rand(1, h, w, generator=g) < 0.5, -1.0, 1.0)
    mask = (torch.rand(1, h, w, generator=g) < 0.75).float()
    interval = torch.tensor([2.5 * 1.06])
    return est.to(dev), gt.to(dev), mask.to(dev), interval.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_depth_metrics needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda")
    results = []
    for h, w in SIZES:
        est, gt, mask, interval = inputs(h, w, dev)
        outputs = {"refined_depth": est}
        hip = lambda: depth_eval.validation_scalars(outputs, gt, mask, interval)            # noqa: E731
        ref = lambda: R.torch_validation_scalars(est, gt, mask, interval)                   # noqa: E731
        a, b = hip(), ref()
        n = int((mask > 0.5).sum())
        worst = max(abs(a[k] - b[k]) / abs(b[k]) for k in R.NAMES)
        assert all(math.isfinite(v) for v in a.values()) and worst <= n * 2.0 ** -24, worst
        for _ in range(args.warmup):
            hip(), ref()
        times = {"hip": [], "torch": []}
        for _ in range(args.repeats):
            for name, fn in (("hip", hip), ("torch", ref)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
        row = {"h": h, "w": w, "masked_pixels": n, "repeats": args.repeats, "warmup": args.warmup, "max_rel_diff": worst}
        for name, ts in times.items():
            row[f"{name}_ms_median"], row[f"{name}_ms_min"], row[f"{name}_ms_max"] = statistics.median(ts), min(ts), max(ts)
        results.append(row)
        print(f"{w} x {h} (B = 1, {n} masked pixels): validation_scalars {row['hip_ms_median']:.3f} ms "
              f"[{row['hip_ms_min']:.3f}, {row['hip_ms_max']:.3f}]   torch ops {row['torch_ms_median']:.3f} ms "
              f"[{row['torch_ms_min']:.3f}, {row['torch_ms_max']:.3f}]   (median [min, max] of {args.repeats}; "
              f"largest relative difference of a scalar {worst:.1e})", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
