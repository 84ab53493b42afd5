"""Device time of the trajectory alignment's RANSAC (cds_mvsnet_amd.tt_eval.ransac_similarity -> cds_ransac_similarity_f64) at
the sizes of Tanks and Temples trajectories, next to the numpy restatement of the same rules on the host, written as
profiles/tt_trajectory.md (a record of what was found, not a threshold).

    python scripts/time_tt_traj.py [--n 150,300,1600] [--iterations 100000] [--k 6] [--repeats 20] [--out profiles/tt_trajectory.md]
    CDS_MVSNET_LIB=cds_mvsnet_amd/_variants/libcdsmvs_hip.ldsstage.so python scripts/time_tt_traj.py --device-only   # an A/B build

Device time: events on the current stream around ``repeats`` back-to-back launches of the two kernels (the C entry point,
without the host read of the result) after a warm-up at the same shape; the median and the minimum of five such windows.  The
wall time of one ``ransac_similarity`` call (upload excluded, the one host read included) is given beside it.  The host
column times ``tests/tt_traj_ref.ransac`` once on the same inputs.  Float64 operations are counted from the shapes: per
hypothesis and point 9 products and 9 sums for T src, 3 differences, 3 products and 2 sums for d2, one compare, one
accumulate."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tt_traj_ref as TR  # noqa: E402
from cds_mvsnet_amd import _lib, tt_eval  # noqa: E402
from cds_mvsnet_amd._lib import check  # noqa: E402
from cds_mvsnet_amd.ops import _stream  # noqa: E402

OPS_PER_POINT = 28
THRESHOLD = 0.2


def device_ms(src, dst, k, H, seed, repeats, windows=5):
    lib = _lib.load()
    ws = torch.empty(((H + 255) // 256) * _lib.RANSAC_RECORD, dtype=torch.float64, device=src.device)
    out = torch.empty(_lib.RANSAC_RECORD, dtype=torch.float64, device=src.device)

    def launch():
        check(lib.cds_ransac_similarity_f64(src.data_ptr(), dst.data_ptr(), src.shape[0], H, k, THRESHOLD, seed, ws.data_ptr(),
                                            ws.numel(), out.data_ptr(), None, None, _stream(src)), "cds_ransac_similarity_f64")
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / repeats)
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="150,300,1600")
    ap.add_argument("--iterations", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tt_trajectory.md"))
    ap.add_argument("--device-only", action="store_true", help="print the device times only: no host restatement, no file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timings need the GPU"
    H, k = args.iterations, args.k
    rows = []
    for n in [int(v) for v in args.n.split(",")]:
        src, dst, S, inl = TR.similarity_data(n, THRESHOLD, 100 + n, extent=10.0)
        s, d = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        med, best = device_ms(s, d, k, H, 0, args.repeats)
        if args.device_only:
            print(f"N {n}: device {med:.4f} ms (min {best:.4f})", flush=True)
            continue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T, info = tt_eval.ransac_similarity(s, d, THRESHOLD, k, H, 0)
        wall = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ref = TR.ransac(src, dst, THRESHOLD, k, H, 0)
        host = time.perf_counter() - t0
        w = ref["index"]
        same = info["count"] == int(ref["count"][w]) and abs(info["rmse"] ** 2 * info["count"] - ref["err2"][w]) <= 1e-9 * ref["err2"][w]
        rate = H * n * OPS_PER_POINT / (med * 1e-3) / 1e12
        rows.append((n, med, best, wall, host, rate, info["count"], int(inl.sum()), same))
        print(f"N {n}: device {med:.3f} ms (min {best:.3f}), call {wall:.2f} ms, numpy {host:.2f} s, {rate:.2f} T fp64 op/s, "
              f"inliers {info['count']} / {int(inl.sum())}, winner as the restatement's: {same}", flush=True)

    if args.device_only:
        return
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"), "ransac.hip", "-Xclang", "-target-feature",
                          "-Xclang", "-packed-fp32-ops"], capture_output=True, text=True).stdout.strip()
    with open(args.out, "w") as f:
        f.write("# Trajectory alignment: `cds_ransac_similarity_f64`\n\n")
        f.write(f"`python scripts/time_tt_traj.py`: H = {H} hypotheses of k = {k}, threshold {THRESHOLD}, 40 % outliers, one MI355X "
                f"({torch.cuda.get_device_name(0)}).  Device time is the median (minimum) of five event-bracketed windows of "
                f"{args.repeats} launches of the two kernels; \"call\" is one `tt_eval.ransac_similarity` with its host read; \"numpy\" is "
                "`tests/tt_traj_ref.ransac` on the same inputs on the host.  The op rate counts "
                f"{OPS_PER_POINT} float64 operations per hypothesis and point (no fused multiply-adds: the library is built without "
                "contraction), the estimate not counted.\n\n")
        f.write("| N | device ms | call ms | numpy s | numpy / device | T fp64 op/s | inliers found / true | winner = restatement's |\n")
        f.write("|---|---|---|---|---|---|---|---|\n")
        for n, med, best, wall, host, rate, got, true, same in rows:
            f.write(f"| {n} | {med:.3f} ({best:.3f}) | {wall:.2f} | {host:.2f} | {host * 1e3 / med:.0f}x | {rate:.2f} | {got} / {true} | {same} |\n")
        f.write("\n## Kernel resources (`scripts/kernel_resources.py ransac.hip`)\n\n```\n" + res + "\n```\n\n")
        f.write("Both kernels use 5120 bytes of LDS per workgroup (the best-record reduction: count, err2 and h of 256 lanes) and no scratch.\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
