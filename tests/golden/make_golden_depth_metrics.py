"""Capture G16: depth-map metrics computed BY THE REFERENCE's own functions on engineered inputs.

Run in the build container only (the reference checkout is not present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_depth_metrics.py

``Thres_metrics`` / ``AbsDepthError_metrics`` (utils.py:134-167, with their two decorators) and ``thres_metrics``
(evaluations/precision.py:8-13) cannot be imported - utils.py pulls in torchvision, precision.py cv2, neither is installed - so the
functions are compiled one by one straight from the reference files with ``ast`` (as make_golden.py:_reference_function does);
nothing is copied.  The drivers around them are this file's own: thresholds and band edges are built from (name, multiplier)
pairs, MAE and RMSE from a masked error vector.  Only data is written: the inputs, the twelve validation scalars and the five precision scalars, for

* case ``a``: B = 2, 48 x 64 (<= 4096 masked pixels per image).  Image 0 has errors in all six ``thres..mm_abserror`` bands,
  image 1 none in the 4-8 and the 14-20 bands (two empty bands -> 0).  Pixels sit EXACTLY on float32(threshold), one ulp above
  and one ulp below, for the thresholds di x 4 and di x 14 (image 0) and di x 2 (image 1), and on 1 / 2 / 4 for the precision
  scalars; the mask holds 0, 1 and values either side of 0.5;
* case ``b``: B = 1 with an all-zero mask (NaN for the means over the mask, 0 for the bands).
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
INTERVAL = np.float32(2.5 * 1.06)                    # DTU's depth interval x interval_scale; di = INTERVAL / 2.65 is not exactly 1
MULT = (2.0, 4.0, 8.0, 14.0, 20.0)


def _reference_function(path, name, glb):
    """Compile ONE top-level function (with its decorators) of a reference file that cannot be imported, into ``glb``."""
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), glb)
    return glb[name]


def reference_metrics():
    glb = {"torch": torch, "np": np, "__builtins__": __builtins__}
    for name in ("make_nograd_func", "compute_metrics_for_each_image", "Thres_metrics", "AbsDepthError_metrics"):
        _reference_function(os.path.join(REF, "utils.py"), name, glb)
    pglb = {"np": np, "__builtins__": __builtins__}
    _reference_function(os.path.join(REF, "evaluations", "precision.py"), "thres_metrics", pglb)
    return glb["Thres_metrics"], glb["AbsDepthError_metrics"], pglb["thres_metrics"]


BAND_NAMES = ("2mm", "4mm", "8mm", "14mm", "20mm", ">20mm")      # the reference's key stems, thresholds di x MULT, last band up to 1e5


def validation_scalars(Thres, AbsErr, est, gt, mask, interval):
    """The twelve scalars of the reference's validation step, from its two compiled metric functions: the overall mean error, the
    share above each threshold di x MULT[k], and the mean error between consecutive edges 0, di x MULT[0], ..., 1e5.  di is batch
    item 0's interval over 2.65 as a Python float; the functions get tensors, a boolean mask and Python-float thresholds."""
    e, g = torch.from_numpy(est), torch.from_numpy(gt)
    sel = torch.from_numpy(mask) > 0.5
    di = float(interval[0]) / 2.65
    edges = [0.0] + [di * m for m in MULT] + [1e5]
    out = {"abs_depth_error": AbsErr(e, g, sel)}
    for k, stem in enumerate(BAND_NAMES[:-1]):
        out[f"thres{stem}_error"] = Thres(e, g, sel, edges[k + 1])
    for k, stem in enumerate(BAND_NAMES):
        out[f"thres{stem}_abserror"] = AbsErr(e, g, sel, [edges[k], edges[k + 1]])
    return {k: float(v) for k, v in out.items()}


def precision_scalars(thres_np, est, gt, mask):
    """Per image MAE and RMSE of the masked float32 errors (numpy means in float32, as a float32 array gives them) and the
    reference's compiled ``thres_metrics`` at 1, 2 and 4; then the mean over the images.  An empty mask gives NaN."""
    rows = []
    for b in range(est.shape[0]):
        sel = mask[b] > 0.5
        if not sel.any():
            rows.append([np.nan] * 5)
            continue
        diff = (est[b] - gt[b])[sel]                         # float32
        rows.append([float(np.abs(diff).mean()), float(np.sqrt(np.square(diff).mean()))] +
                    [thres_np(est[b], gt[b], sel, t) for t in (1, 2, 4)])
    return np.asarray(rows, np.float64).mean(axis=0)


def _ulps(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(np.inf))]


def case_a():
    rs = np.random.RandomState(16)
    B, h, w = 2, 48, 64
    di = float(INTERVAL) / 2.65
    thr = [np.float32(di * m) for m in MULT]                                 # the float32 thresholds ATen compares against
    gt = (rs.rand(B, h, w) * 400 + 450).astype(np.float32)
    mask = (rs.rand(B, h, w) > 0.3).astype(np.float32)
    mask[rs.rand(B, h, w) < 0.02] = 0.5                                      # not selected (> 0.5 is strict)
    mask[rs.rand(B, h, w) < 0.02] = 0.75
    # errors: image 0 anywhere in [0, 30 di] (all six bands), image 1 only in the bands 0-2, 2-4, 8-14 and > 20 (margins keep the
    # rounding of gt + e away from the band edges)
    err = np.zeros((B, h, w))
    err[0] = rs.rand(h, w) * 30 * di
    lo = np.array([0.0, 2 * di, 8 * di, 20 * di]) + 0.01
    hi = np.array([2 * di, 4 * di, 14 * di, 40 * di]) - 0.01
    pick = rs.randint(0, 4, size=(h, w))
    err[1] = lo[pick] + rs.rand(h, w) * (hi - lo)[pick]
    sign = np.where(rs.rand(B, h, w) < 0.5, -1.0, 1.0)
    est = (gt.astype(np.float64) + sign * err).astype(np.float32)
    # pixels exactly on / one ulp either side of a threshold: gt = 0 (or est = 0) makes e the chosen float32 bit for bit
    spots = [(0, thr[1]), (0, thr[3]), (1, thr[0]), (0, 1.0), (0, 2.0), (0, 4.0)]
    x = 0
    for b, t in spots:
        for k, v in enumerate(_ulps(t)):
            for flip in (0, 1):
                y = 3 + 2 * k + flip
                mask[b, y, x] = 1.0
                if flip:
                    est[b, y, x], gt[b, y, x] = 0.0, v
                else:
                    est[b, y, x], gt[b, y, x] = -v, 0.0
        x += 3
    return est, gt, mask, np.array([INTERVAL, np.float32(9.0)], np.float32)  # item 1's interval must be ignored


def case_b():
    rs = np.random.RandomState(17)
    gt = (rs.rand(1, 48, 64) * 400 + 450).astype(np.float32)
    est = (gt + rs.randn(1, 48, 64).astype(np.float32) * 5).astype(np.float32)
    return est, gt, np.zeros((1, 48, 64), np.float32), np.array([INTERVAL], np.float32)


def main():
    Thres, AbsErr, thres_np = reference_metrics()
    sys.path.insert(0, os.path.dirname(HERE))
    import depth_eval_ref as R
    out = {}
    for tag, (est, gt, mask, interval) in (("a", case_a()), ("b", case_b())):
        val = validation_scalars(Thres, AbsErr, est, gt, mask, interval)
        prec = precision_scalars(thres_np, est, gt, mask)
        assert tuple(val) == R.NAMES
        out.update({f"{tag}_est": est, f"{tag}_gt": gt, f"{tag}_mask": mask, f"{tag}_interval": interval,
                    f"{tag}_validation": np.array([val[k] for k in R.NAMES], np.float64), f"{tag}_precision": prec})
        print(tag, "masked pixels per image:", [(m > 0.5).sum() for m in mask])
        for k in R.NAMES:
            print(f"  {k:22s} {val[k]!r}")
        print("  precision", prec)
    # what the fixture is for: every band filled in image 0, two empty in image 1
    sums = R.metric_sums(out["a_est"], out["a_gt"], out["a_mask"], [float(INTERVAL) / 2.65 * m for m in MULT], 1e5)
    counts = sums[:, 3 + 5::2]
    assert (counts[0] > 0).all() and (counts[1] == 0).sum() == 2, counts
    assert max((m > 0.5).sum() for m in out["a_mask"]) <= 4096
    out["names"] = np.array(R.NAMES)
    path = os.path.join(HERE, "g16_depth_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"g16_depth_metrics: {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
