"""Test infrastructure: float64 numpy restatement of cds_mvsnet_amd.depth_eval / csrc/depth_metrics.hip - the sums of kernel A, the
three metric families (utils.py:134-167 as trainer/trainer.py:140-164 calls them, evaluations/precision.py:8-13,87-91), OpenCV's
INTER_NEAREST index rule and the ground-truth pyramid of kernel B - plus the twelve validation scalars written in torch ops the
reference's way (one masked index / compare / mean pass and one host read per scalar), which the GPU tests and
scripts/time_depth_metrics.py run on device tensors.

The error e = |est - gt| and every comparison are float32 (what the reference computes); only the accumulation is float64."""
import numpy as np
import torch

MULTIPLIERS = (2.0, 4.0, 8.0, 14.0, 20.0)
CAP = 1e5
NAMES = ("abs_depth_error",
         "thres2mm_error", "thres4mm_error", "thres8mm_error", "thres14mm_error", "thres20mm_error",
         "thres2mm_abserror", "thres4mm_abserror", "thres8mm_abserror", "thres14mm_abserror", "thres20mm_abserror",
         "thres>20mm_abserror")
PRECISION_NAMES = ("MAE", "RMSE", "thresh1mm_error", "thresh2mm_error", "thresh4mm_error")


def _errors(est, gt, mask):
    """float32 errors of the masked pixels of ONE image, in raster order."""
    est, gt = np.asarray(est, np.float32), np.asarray(gt, np.float32)
    sel = np.asarray(mask, np.float32) > np.float32(0.5)
    return np.abs(est[sel] - gt[sel]).astype(np.float32)


def _thr_rows(thr, B):
    t = np.asarray(thr, np.float64).astype(np.float32)
    return np.broadcast_to(t, (B, t.shape[-1])) if t.ndim == 1 else t


def metric_sums(est, gt, mask, thr, cap):
    """[B, 3T+5] float64: n, sum e, sum e^2, #{e > thr_t}, then (count, sum e) of the T+1 inclusive bands."""
    B = est.shape[0]
    thr = _thr_rows(thr, B)
    T = thr.shape[1]
    out = np.zeros((B, 3 * T + 5), np.float64)
    for b in range(B):
        e = _errors(est[b], gt[b], mask[b])
        e64 = e.astype(np.float64)
        out[b, 0], out[b, 1], out[b, 2] = e.size, e64.sum(), (e64 * e64).sum()
        for t in range(T):
            out[b, 3 + t] = np.count_nonzero(e > thr[b, t])
        edges = [np.float32(0.0)] + [thr[b, t] for t in range(T)] + [np.float32(cap)]
        for k in range(T + 1):
            sel = (e >= edges[k]) & (e <= edges[k + 1])
            out[b, 3 + T + 2 * k] = np.count_nonzero(sel)
            out[b, 3 + T + 2 * k + 1] = e64[sel].sum()
    return out


def thres_metric(est, gt, mask, thr):
    """Thres_metrics: mean over the batch of the share of masked pixels with e > float32(thr); NaN for an empty mask."""
    vals = []
    for b in range(est.shape[0]):
        e = _errors(est[b], gt[b], mask[b])
        vals.append(np.count_nonzero(e > np.float32(thr)) / e.size if e.size else np.nan)
    return float(np.mean(vals))


def abs_error(est, gt, mask, band=None):
    """AbsDepthError_metrics: mean over the batch of the mean masked error, inside the inclusive band if given (empty band: 0)."""
    vals = []
    for b in range(est.shape[0]):
        e = _errors(est[b], gt[b], mask[b])
        if band is not None:
            e = e[(e >= np.float32(band[0])) & (e <= np.float32(band[1]))]
            if e.size == 0:
                vals.append(0.0)
                continue
        vals.append(e.astype(np.float64).mean() if e.size else np.nan)
    return float(np.mean(vals))


def validation_scalars(est, gt, mask, interval0):
    """The twelve scalars of trainer.py:140-164; interval0 = depth_interval[0] (di = interval0 / 2.65 as a Python float)."""
    di = float(interval0) / 2.65
    t = [di * m for m in MULTIPLIERS]
    vals = [abs_error(est, gt, mask)] + [thres_metric(est, gt, mask, x) for x in t]
    vals += [abs_error(est, gt, mask, b) for b in zip([0.0] + t, t + [CAP])]
    return dict(zip(NAMES, vals))


def precision_scalars(est, gt, mask):
    """precision.py:87-91 per image, averaged over the images (Evaluation.eval's DictAverageMeter)."""
    if est.ndim == 2:
        est, gt, mask = est[None], gt[None], mask[None]
    rows = []
    for b in range(est.shape[0]):
        e = _errors(est[b], gt[b], mask[b])
        e64 = e.astype(np.float64)
        if e.size == 0:
            rows.append([np.nan] * 5)
            continue
        rows.append([e64.mean(), np.sqrt((e64 * e64).mean())] + [1.0 - np.count_nonzero(e > np.float32(t)) / e.size for t in (1, 2, 4)])
    return dict(zip(PRECISION_NAMES, (float(v) for v in np.mean(np.asarray(rows, np.float64), axis=0))))


def nearest_index(n_dst, n_src):
    """OpenCV INTER_NEAREST: floor(i * (1 / (n_dst / n_src))) clipped to n_src - 1, float64."""
    inv = 1.0 / (n_dst / n_src)
    return np.array([min(int(np.floor(i * inv)), n_src - 1) for i in range(n_dst)], np.int64)


def pyramid(src, rows, cols, levels, mask_src=None, mask_thresh=10):
    """([depth level 0..levels-1], [mask ...]): level 0 = src[rows][:, cols], level k = every 2^k-th pixel of it."""
    src = np.asarray(src, np.float32)
    d0 = src[np.asarray(rows)][:, np.asarray(cols)]
    if mask_src is not None:
        m0 = (np.asarray(mask_src)[np.asarray(rows)][:, np.asarray(cols)].astype(np.int64) > mask_thresh).astype(np.float32)
    else:
        m0 = (d0 > 0).astype(np.float32)
    return [d0[::1 << k, ::1 << k].copy() for k in range(levels)], [m0[::1 << k, ::1 << k].copy() for k in range(levels)]


def dtu_tables(Hs, Ws, crop=(512, 640)):
    """dtu_yao.py:79-94: INTER_NEAREST to (Hs // 2, Ws // 2), then the centre crop."""
    rows, cols = nearest_index(Hs // 2, Hs), nearest_index(Ws // 2, Ws)
    y0, x0 = (Hs // 2 - crop[0]) // 2, (Ws // 2 - crop[1]) // 2
    return rows[y0:y0 + crop[0]], cols[x0:x0 + crop[1]]


def blended_tables(Hs, Ws, crop=(576, 768)):
    """blended_dataset.py:79-84: the centre crop alone."""
    y0, x0 = (Hs - crop[0]) // 2, (Ws - crop[1]) // 2
    return np.arange(Hs)[y0:y0 + crop[0]], np.arange(Ws)[x0:x0 + crop[1]]


# ---- the same metrics in torch ops, one pass and one host read per metric (device tensors welcome) ----------------------------
def _masked_errors(est, gt, sel):
    """Per image the float32 error vector of the selected pixels."""
    return [(est[b] - gt[b]).abs()[sel[b]] for b in range(est.shape[0])]


def _share_above(errors, thr):
    return torch.stack([(e > thr).float().mean() for e in errors]).mean()


def _mean_inside(errors, lo=None, hi=None):
    vals = []
    for e in errors:
        if lo is not None:
            inside = (e >= lo) & (e <= hi)
            vals.append(e[inside].mean() if bool(inside.any()) else e.new_zeros(()))
        else:
            vals.append(e.mean())
    return torch.stack(vals).mean()


@torch.no_grad()
def torch_validation_scalars(est, gt, mask, depth_interval):
    """The twelve validation scalars in torch ops, metric by metric as the reference's trainer asks for them: est, gt [B,H,W], mask
    float [B,H,W], depth_interval [B].  Every metric gathers the masked errors again, compares and averages per image in float32 and
    is read back on its own (thirteen host reads with the interval), which is the cost the fused kernel removes."""
    sel = mask > 0.5
    di = depth_interval[0].item() / 2.65
    edges = [0.0] + [di * k for k in MULTIPLIERS] + [CAP]
    vals = [_mean_inside(_masked_errors(est, gt, sel)).item()]
    vals += [_share_above(_masked_errors(est, gt, sel), t).item() for t in edges[1:-1]]
    vals += [_mean_inside(_masked_errors(est, gt, sel), lo, hi).item() for lo, hi in zip(edges[:-1], edges[1:])]
    return dict(zip(NAMES, vals))
