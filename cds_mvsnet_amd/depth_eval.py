"""How good is a depth map?  The reference answers in two places, both restated here on the GPU:

* validation (``trainer/trainer.py:102-181`` with the metric functions of ``utils.py:134-167``): ``abs_depth_error``, five
  ``thresNmm_error`` and six banded ``thres...mm_abserror`` of the refined depth against the stage-4 ground truth, next to the
  loss and the depth loss - :func:`validation_scalars`, :func:`validate`;
* depth precision (``evaluations/precision.py``): MAE, RMSE and the share of pixels within 1 / 2 / 4 mm of saved
  ``depth_est/*.pfm`` (and the per-stage ``depth_stage1..3`` that ``infer --save_stages`` writes) against DTU's ``Depths_raw`` -
  :func:`precision_scalars` and the command line

      python -m cds_mvsnet_amd.depth_eval --gtpath <.../Depths_raw> --outdir <infer outdir> --testlist <list> \
          [--folders depth_est,depth_stage1,depth_stage2,depth_stage3] [--json out.json]

One kernel pass (``ops.depth_metric_sums``, csrc/depth_metrics.hip) writes every sum these scalars are made of, for all images of a
batch; the scalars are formed on the host from ONE device-to-host read.  :func:`read_gt_ms` prepares the multi-scale ground truth
of the two training datasets with one gather launch (``ops.gt_pyramid``).

Rules:

* the error ``e = |est - gt|`` and every comparison are float32, against the threshold rounded to float32 - what ATen does with a
  Python-float threshold: with ``thr = 0.2`` an error of ``float32(0.2)`` (which is larger than the double 0.2) is NOT counted as
  exceeding it;
* the bands ``[lo, hi]`` of the ``abserror`` family include both ends (utils.py:164): an error exactly on a threshold is in two bands;
* per-image values are averaged over the batch (``compute_metrics_for_each_image``); an empty band gives 0; an EMPTY MASK gives NaN
  for ``abs_depth_error`` and the ``thres*_error`` family (the mean of nothing), as in the reference, and the NaN propagates
  through batch and sample means;
* ``di = depth_interval[0] / 2.65`` comes from batch item 0 alone, in double precision (a Python float in the reference), and
  serves every item of the batch;
* resizes follow OpenCV's ``INTER_NEAREST`` index rule (:func:`nearest_index`).  OpenCV is not installed here, so that rule is
  restated from its documented formula and could not be checked against ``cv2`` itself.

The inputs must be float32 ROCm tensors; there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import mvs_io, ops
from .losses import final_loss

Tensor = torch.Tensor

VALIDATION_MULTIPLIERS = (2.0, 4.0, 8.0, 14.0, 20.0)          # thresholds in units of di (trainer.py:146-163)
VALIDATION_CAP = 1e5                                          # upper end of the last band (trainer.py:163)
VALIDATION_NAMES = ("abs_depth_error",
                    "thres2mm_error", "thres4mm_error", "thres8mm_error", "thres14mm_error", "thres20mm_error",
                    "thres2mm_abserror", "thres4mm_abserror", "thres8mm_abserror", "thres14mm_abserror", "thres20mm_abserror",
                    "thres>20mm_abserror")
PRECISION_THRESHOLDS = (1.0, 2.0, 4.0)                        # mm (precision.py:89-91)
PRECISION_NAMES = ("MAE", "RMSE", "thresh1mm_error", "thresh2mm_error", "thresh4mm_error")
LAYOUTS = {"dtu": {"halve": True, "crop": (512, 640)},        # dtu_yao.py:79-94: half size, centre crop; mask png > 10
           "blended": {"halve": False, "crop": (576, 768)}}   # blended_dataset.py:79-84: centre crop; mask = depth > 0
DTU_MASK_THRESHOLD = 10


# ---------------------------------------------------------------------------------------------------------------------
# host index tables
def nearest_index(n_dst: int, n_src: int) -> np.ndarray:
    """Source index of every destination index when ``n_src`` samples are resized to ``n_dst`` the way OpenCV's ``INTER_NEAREST``
    does: ``min(floor(i * (1.0 / (n_dst / n_src))), n_src - 1)`` in float64 - OpenCV inverts the FORWARD scale instead of
    dividing ``n_src / n_dst``, and the two can land on different pixels where the product is an integer (1600 -> 864 at i = 27:
    49 here, 50 with ``i * (n_src / n_dst)``, which is what ``mvs_io.nearest_resize`` computes for the side outputs of infer;
    1080 -> 600 at i = 15: 26 against 27.  For 1600 -> 1152 and 1200 -> 864 both rules give the same table: the two scale
    factors round to the same double there).
    ``cv2`` is not installed in this project's environment: the rule is restated from OpenCV's formula and has NOT been compared
    with a cv2 run.  -> int64 [n_dst]."""
    n_dst, n_src = int(n_dst), int(n_src)
    if n_dst < 1 or n_src < 1:
        raise ValueError(f"nearest_index: sizes must be positive, got {n_dst}, {n_src}")
    inv = 1.0 / (float(n_dst) / float(n_src))
    return np.minimum(np.floor(np.arange(n_dst, dtype=np.float64) * inv).astype(np.int64), n_src - 1)


def resize_tables(Hs: int, Ws: int, h: int, w: int) -> Tuple[np.ndarray, np.ndarray]:
    """(rows [h], cols [w]) of ``cv2.resize(src, (w, h), interpolation=INTER_NEAREST)`` for an Hs x Ws source."""
    return nearest_index(h, Hs), nearest_index(w, Ws)


def gt_tables(Hs: int, Ws: int, layout: str, crop: Optional[Tuple[int, int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(rows, cols) of the reference's ``prepare_img`` for an Hs x Ws ground-truth file, resize and centre crop composed into one
    gather: ``layout="dtu"`` halves with INTER_NEAREST to (Hs // 2, Ws // 2) and crops 512 x 640 from (h - 512) // 2,
    (w - 640) // 2 (dtu_yao.py:79-94); ``layout="blended"`` crops 576 x 768 the same way (blended_dataset.py:79-84).
    ``crop`` = (height, width) replaces the layout's crop size.  A source smaller than the crop raises."""
    if layout not in LAYOUTS:
        raise ValueError(f"unknown ground-truth layout {layout!r} (expected one of {sorted(LAYOUTS)})")
    rule = LAYOUTS[layout]
    if rule["halve"]:
        rows, cols = resize_tables(Hs, Ws, Hs // 2, Ws // 2) if Hs >= 2 and Ws >= 2 else (np.zeros(0, np.int64),) * 2
    else:
        rows, cols = np.arange(Hs, dtype=np.int64), np.arange(Ws, dtype=np.int64)
    th, tw = (int(crop[0]), int(crop[1])) if crop is not None else rule["crop"]
    h, w = rows.size, cols.size
    if th < 1 or tw < 1 or h < th or w < tw:
        raise ValueError(f"{layout}: a {Hs} x {Ws} file gives {h} x {w} before the crop, smaller than the {th} x {tw} crop")
    y0, x0 = (h - th) // 2, (w - tw) // 2
    return rows[y0:y0 + th].copy(), cols[x0:x0 + tw].copy()


# ---------------------------------------------------------------------------------------------------------------------
# scalars from the kernel's sums (host, float64)
def _per_image(sums: np.ndarray, T: int) -> Dict[str, np.ndarray]:
    """sums [..., 3T+5] (ops.depth_metric_sums) -> per image: n, mae, rmse [...], thres [..., T], band [..., T+1]."""
    s = np.asarray(sums, dtype=np.float64)
    n = s[..., 0]
    cnt, tot = s[..., 3 + T::2], s[..., 4 + T::2]
    with np.errstate(divide="ignore", invalid="ignore"):
        mae = s[..., 1] / n                                   # 0 / 0 = NaN: the mean over an empty mask
        rmse = np.sqrt(s[..., 2] / n)
        thres = s[..., 3:3 + T] / n[..., None]
        band = np.where(cnt > 0, tot / np.where(cnt > 0, cnt, 1.0), 0.0)      # an empty band is 0 (utils.py:165-166)
    return {"n": n, "mae": mae, "rmse": rmse, "thres": thres, "band": band}


def _validation_from_sums(sums: np.ndarray) -> Dict[str, float]:
    """sums [B, 20] with the five validation thresholds -> the reference's twelve scalars, each the mean over the batch."""
    m = _per_image(sums, len(VALIDATION_MULTIPLIERS))
    vals = [m["mae"].mean()] + list(m["thres"].mean(axis=0)) + list(m["band"].mean(axis=0))
    return {k: float(v) for k, v in zip(VALIDATION_NAMES, vals)}


def _precision_from_sums(sums: np.ndarray) -> Dict[str, float]:
    """sums [..., 14] with thresholds 1, 2, 4 -> MAE, RMSE, thresh{1,2,4}mm_error, each the mean over all leading axes."""
    m = _per_image(np.asarray(sums).reshape(-1, 3 * len(PRECISION_THRESHOLDS) + 5), len(PRECISION_THRESHOLDS))
    within = 1.0 - m["thres"]                                 # precision.py:13: the share NOT exceeding, under an "_error" name
    vals = [m["mae"].mean(), m["rmse"].mean()] + list(within.mean(axis=0))
    return {k: float(v) for k, v in zip(PRECISION_NAMES, vals)}


def _as_batch(est: Tensor, gt: Tensor, mask: Tensor, what: str) -> Tuple[Tensor, Tensor, Tensor]:
    for name, t in (("est", est), ("gt", gt), ("mask", mask)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: {name} must be a ROCm (cuda) tensor; there is no CPU fallback")
    if mask.dtype == torch.bool:
        mask = mask.float()
    out = []
    for name, t in (("est", est), ("gt", gt), ("mask", mask)):
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32 (mask: float32 or bool), got {t.dtype}")
        t = t.detach()
        out.append((t.unsqueeze(0) if t.dim() == 2 else t).contiguous())
    return out[0], out[1], out[2]


def _sums(est: Tensor, gt: Tensor, mask: Tensor, thr, cap: float, what: str) -> Tensor:
    est, gt, mask = _as_batch(est, gt, mask, what)
    with torch.cuda.device(est.device):
        return ops.depth_metric_sums(est, gt, mask, thr, cap)


def depth_metrics(est: Tensor, gt: Tensor, mask: Tensor, thresholds: Sequence[float], cap: float = VALIDATION_CAP) -> Dict[str, object]:
    """est, gt [B,h,w] (or [h,w]) float32, mask the same shape (float32, > 0.5 selects; or bool) on the device; ``thresholds``: T <= 8
    ascending values, [T] for every image or [B][T].  -> {"abs_depth_error": mean |est - gt| over the mask, "rmse",
    "thres_error": [T] share of masked pixels with error > t, "band_abserror": [T+1] mean error inside [0,t0], [t0,t1], ...,
    [t_{T-1},cap] (both ends included), "pixels": masked pixels per image}.  Each value is computed per image and averaged over the
    batch.  An empty band gives 0; an empty mask gives NaN for ``abs_depth_error``, ``rmse`` and ``thres_error``, as the
    reference's mean of nothing does.  One kernel pass, one device-to-host read."""
    sums = _sums(est, gt, mask, thresholds, cap, "depth_metrics").cpu().numpy()
    T = (sums.shape[1] - 5) // 3
    m = _per_image(sums, T)
    return {"abs_depth_error": float(m["mae"].mean()), "rmse": float(m["rmse"].mean()),
            "thres_error": [float(v) for v in m["thres"].mean(axis=0)],
            "band_abserror": [float(v) for v in m["band"].mean(axis=0)], "pixels": [int(v) for v in m["n"]]}


def _validation_thresholds(depth_interval, B: int, device):
    """di = depth_interval[0] / 2.65 in double precision, thresholds di x {2, 4, 8, 14, 20}: a device interval stays on the device
    (float64 arithmetic there is the Python-float arithmetic of the reference, bit for bit; no host read), anything else is
    computed on the host."""
    if isinstance(depth_interval, torch.Tensor) and depth_interval.is_cuda:
        di = depth_interval.detach().reshape(-1)[0].double() / 2.65
        mult = torch.tensor(VALIDATION_MULTIPLIERS, dtype=torch.float64, device=depth_interval.device)
        return (di * mult).float().unsqueeze(0).expand(B, len(VALIDATION_MULTIPLIERS)).contiguous().to(device)
    first = depth_interval.reshape(-1)[0] if isinstance(depth_interval, (torch.Tensor, np.ndarray)) else \
        (depth_interval[0] if isinstance(depth_interval, (list, tuple)) else depth_interval)
    di = float(first) / 2.65
    return [di * m for m in VALIDATION_MULTIPLIERS]


def _validation_sums(outputs, depth_gt, mask, depth_interval) -> Tensor:
    est = outputs["refined_depth"]
    gt = depth_gt["stage4"] if isinstance(depth_gt, dict) else depth_gt
    msk = mask["stage4"] if isinstance(mask, dict) else mask
    est, gt, msk = _as_batch(est, gt, msk, "validation_scalars")
    thr = _validation_thresholds(depth_interval, est.shape[0], est.device)
    with torch.cuda.device(est.device):
        return ops.depth_metric_sums(est, gt, msk, thr, VALIDATION_CAP)


def validation_scalars(outputs, depth_gt, mask, depth_interval) -> Dict[str, float]:
    """The twelve metric scalars of the reference's validation step (trainer.py:140-164) for ``outputs["refined_depth"]`` [B,H,W]
    against the stage-4 ground truth: ``depth_gt`` / ``mask`` are the ``{"stage1".."stage4"}`` dicts of a sample or the stage-4
    tensors themselves; ``depth_interval`` [B] (tensor on either side, array or list): ``di = depth_interval[0] / 2.65`` from
    batch item 0, thresholds ``di x {2, 4, 8, 14, 20}``.  Keys: :data:`VALIDATION_NAMES`."""
    return _validation_from_sums(_validation_sums(outputs, depth_gt, mask, depth_interval).cpu().numpy())


def precision_scalars(est: Tensor, gt: Tensor, mask: Tensor) -> Dict[str, float]:
    """precision.py:87-91 for est, gt, mask [h,w] or [B,h,w] (mask > 0.5 selects): ``MAE``, ``RMSE`` and
    ``thresh{1,2,4}mm_error = 1 - mean(e > t)`` - under that name the reference reports the share of pixels WITHIN t; the
    misleading key is kept so the numbers line up with its printout.  Mean over the images."""
    return _precision_from_sums(_sums(est, gt, mask, PRECISION_THRESHOLDS, VALIDATION_CAP, "precision_scalars").cpu().numpy())


def validate(model: torch.nn.Module, samples: Iterable[Dict[str, object]], temperature: float,
             dlossw: Optional[Sequence[float]] = None) -> Dict[str, float]:
    """The reference's ``_valid_epoch`` (trainer.py:102-181) over ``samples``, an iterable of the dicts ``train.train_step`` takes
    ({imgs, proj_matrices, depth_values, depth: {stageK}, mask: {stageK}}, tensors on the model's device): ``model.eval()`` under
    ``torch.no_grad()``, forward through ``model(...)``, ``losses.final_loss`` on the inference outputs (they carry ``depth`` and
    ``norm_curv``; no feature-distance term outside training), the twelve metrics of :func:`validation_scalars`.  Everything a
    sample yields stays on the device; ONE device-to-host read at the end fetches all of it.  -> the mean over the samples of
    ``loss``, ``depth_loss`` and the twelve metrics (``DictAverageMeter``); a NaN (a sample with an empty mask) propagates.  The
    model's training / eval mode is restored."""
    was_training = model.training
    if was_training:
        model.eval()
    rows: List[Tensor] = []
    batches: List[int] = []
    try:
        with torch.no_grad():
            for sample in samples:
                imgs = sample["imgs"]
                dv = sample["depth_values"]
                outputs = model(imgs, sample["proj_matrices"], dv, temperature=temperature)
                dvd = dv.to(imgs.device)
                interval = (dvd[:, 1] - dvd[:, 0]).float()
                kw = {"depth_interval": interval}
                if dlossw is not None:
                    kw["dlossw"] = list(dlossw)
                with torch.cuda.device(imgs.device):
                    loss, depth_loss = final_loss(outputs, sample["depth"], sample["mask"], **kw)
                sums = _validation_sums(outputs, sample["depth"], sample["mask"], interval)
                rows.append(torch.cat((torch.stack((loss.detach().reshape(()), depth_loss.detach().reshape(()))).double(),
                                       sums.reshape(-1))))
                batches.append(int(sums.shape[0]))
    finally:
        if was_training:
            model.train()
    if not rows:
        raise ValueError("validate: no samples")
    flat = torch.cat(rows).cpu().numpy()                      # the one device-to-host read
    total: Dict[str, float] = {}
    off = 0
    nf = 3 * len(VALIDATION_MULTIPLIERS) + 5
    for B in batches:
        rec = flat[off:off + 2 + B * nf]
        off += 2 + B * nf
        scal = {"loss": float(rec[0]), "depth_loss": float(rec[1])}
        scal.update(_validation_from_sums(rec[2:].reshape(B, nf)))
        for k, v in scal.items():
            total[k] = total.get(k, 0.0) + v
    return {k: v / len(batches) for k, v in total.items()}


# ---------------------------------------------------------------------------------------------------------------------
# ground truth from disk
def _read_mask_png(path: str) -> np.ndarray:
    """A mask image as uint8 [H,W]; an image of another depth is thresholded here (> 10 -> 255) so the kernel's rule still holds."""
    from PIL import Image
    a = np.array(Image.open(path))                            # a writable copy: torch.from_numpy wants one
    if a.ndim != 2:
        raise ValueError(f"{path}: expected a single-channel mask image, got shape {a.shape}")
    if a.dtype != np.uint8:
        a = np.where(a.astype(np.float64) > DTU_MASK_THRESHOLD, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(a)


def read_gt_ms(depth_pfm: str, mask_png: Optional[str], layout: str, device, levels: int = 4,
               crop: Optional[Tuple[int, int]] = None, tables: Optional[Dict] = None) -> Tuple[Dict[str, Tensor], Dict[str, Tensor]]:
    """Multi-scale ground truth of one view as the reference's datasets prepare it, through one gather launch:
    ``layout="dtu"``: ``depth_pfm`` = Depths_raw/.../depth_map_%04d.pfm, ``mask_png`` = depth_visual_%04d.png; half size
    (INTER_NEAREST, :func:`nearest_index`), centre crop 512 x 640, mask = png > 10 (dtu_yao.py:79-128);
    ``layout="blended"``: ``depth_pfm`` = rendered_depth_maps/%08d.pfm, ``mask_png`` None; centre crop 576 x 768, mask = depth > 0
    (blended_dataset.py:79-120).  ``crop`` = (height, width) overrides the crop size.  ``tables``: a dict the caller keeps between calls
    (a loader reads thousands of views of one size): the device index tables are built and uploaded once per (file size, layout,
    crop, device) and reused from it.  -> (depth, mask): dicts ``stage{levels}``
    (the cropped resolution) down to ``stage1`` (every 2^(levels-1)-th pixel), float32 on ``device``."""
    if layout not in LAYOUTS:
        raise ValueError(f"unknown ground-truth layout {layout!r} (expected one of {sorted(LAYOUTS)})")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("read_gt_ms prepares the ground truth on the GPU only (device cuda[:N])")
    depth = mvs_io.read_pfm(depth_pfm)[0]
    if depth.ndim != 2:
        raise ValueError(f"{depth_pfm}: expected a single-channel depth map")
    mask8 = None
    if layout == "dtu":
        if mask_png is None:
            raise ValueError("read_gt_ms: the dtu layout needs the depth_visual mask image")
        mask8 = _read_mask_png(mask_png)
        if mask8.shape != depth.shape:
            raise ValueError(f"{mask_png}: mask is {mask8.shape}, the depth map {depth.shape}")
    elif mask_png is not None:
        raise ValueError("read_gt_ms: the blended layout takes its mask from the depth map (mask_png must be None)")
    with torch.cuda.device(dev):
        key = (depth.shape, layout, tuple(crop) if crop is not None else None, str(dev))
        if tables is not None and key in tables:
            rows, cols = tables[key]
        else:
            rows, cols = ops.index_tables(*gt_tables(depth.shape[0], depth.shape[1], layout, crop), depth.shape[0], depth.shape[1], dev)
            if tables is not None:
                tables[key] = (rows, cols)
        d = torch.from_numpy(np.ascontiguousarray(depth)).to(dev)
        m = torch.from_numpy(mask8).to(dev) if mask8 is not None else None
        depths, masks = ops.gt_pyramid(d, rows, cols, levels=levels, mask_src=m, mask_thresh=DTU_MASK_THRESHOLD)
    names = [f"stage{levels - k}" for k in range(levels)]
    return dict(zip(names, depths)), dict(zip(names, masks))


# ---------------------------------------------------------------------------------------------------------------------
# command line: evaluations/precision.py
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m cds_mvsnet_amd.depth_eval",
                                 description="depth precision (MAE, RMSE, share within 1 / 2 / 4 mm) of saved depth maps against "
                                             "DTU Depths_raw, on the GPU")
    ap.add_argument("--gtpath", required=True, help="the Depths_raw folder (<scan>/depth_map_%%04d.pfm, depth_visual_%%04d.png)")
    ap.add_argument("--outdir", required=True, help="the infer --outdir (<scan>/<folder>/%%08d.pfm)")
    ap.add_argument("--testlist", required=True, help="file with one scan per line")
    ap.add_argument("--folders", default="depth_est",
                    help="comma-separated sub-folders to score, e.g. depth_est,depth_stage1,depth_stage2,depth_stage3")
    ap.add_argument("--json", help="write the per-folder results here")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    args.folders = [f.strip() for f in args.folders.split(",") if f.strip()]
    if not args.folders:
        ap.error("--folders names no folder")
    return args


def _folder_jobs(gtpath: str, outdir: str, scans: Sequence[str], folder: str) -> List[Tuple[str, str, str]]:
    """(estimate, ground-truth depth, ground-truth mask) of every *.pfm index in each scan's folder (precision.py:20-35); a missing
    file raises before anything is scored."""
    jobs = []
    for scan in scans:
        est_dir = os.path.join(outdir, scan, folder)
        if not os.path.isdir(est_dir):
            raise FileNotFoundError(f"{scan}: {est_dir} not found")
        stems = sorted(int(os.path.splitext(f)[0]) for f in os.listdir(est_dir)
                       if f.endswith(".pfm") and os.path.splitext(f)[0].isdigit())
        for idx in stems:
            est = os.path.join(est_dir, f"{idx:08d}.pfm")
            gt = os.path.join(gtpath, scan, f"depth_map_{idx:04d}.pfm")
            msk = os.path.join(gtpath, scan, f"depth_visual_{idx:04d}.png")
            for p in (est, gt, msk):
                if not os.path.isfile(p):
                    raise FileNotFoundError(f"{scan}/{folder} view {idx}: {p} not found")
            jobs.append((est, gt, msk))
    return jobs


def score_files(jobs: Sequence[Tuple[str, str, str]], device) -> Dict[str, float]:
    """Evaluation.eval (precision.py:79-93) over (estimate, gt depth, gt mask) files: ground truth and mask are resized with
    INTER_NEAREST to the ESTIMATE'S OWN size (precision.py has the caller pass that size), every image is scored on its own and
    the five scalars are averaged over all images.  One device-to-host read for the whole list."""
    dev = torch.device(device)
    sums = []
    tables: Dict[tuple, Tuple[Tensor, Tensor]] = {}
    with torch.cuda.device(dev):
        for est_p, gt_p, mask_p in jobs:
            est = mvs_io.read_pfm(est_p)[0]
            gt = mvs_io.read_pfm(gt_p)[0]
            if est.ndim != 2 or gt.ndim != 2:
                raise ValueError(f"{est_p} / {gt_p}: expected single-channel depth maps")
            mask8 = _read_mask_png(mask_p)
            if mask8.shape != gt.shape:
                raise ValueError(f"{mask_p}: mask is {mask8.shape}, the depth map {gt.shape}")
            key = (gt.shape, est.shape)
            if key not in tables:                          # one upload per pair of sizes, not per image
                tables[key] = ops.index_tables(*resize_tables(gt.shape[0], gt.shape[1], est.shape[0], est.shape[1]),
                                               gt.shape[0], gt.shape[1], dev)
            rows, cols = tables[key]
            d, m = ops.gt_pyramid(torch.from_numpy(np.ascontiguousarray(gt)).to(dev), rows, cols, levels=1,
                                  mask_src=torch.from_numpy(mask8).to(dev), mask_thresh=DTU_MASK_THRESHOLD)
            e = torch.from_numpy(np.ascontiguousarray(est)).to(dev)
            sums.append(ops.depth_metric_sums(e.unsqueeze(0), d[0].unsqueeze(0), m[0].unsqueeze(0), PRECISION_THRESHOLDS,
                                              VALIDATION_CAP))
        if not sums:
            raise ValueError("no depth maps to score")
        host = torch.cat(sums).cpu().numpy()
    out = _precision_from_sums(host)
    out["images"] = len(jobs)
    return out


def main(argv: Optional[Sequence[str]] = None) -> Dict[str, object]:
    args = parse_args(argv)
    dev = torch.device(args.device)
    if dev.type != "cuda":
        raise SystemExit("depth_eval runs on the GPU only (--device cuda[:N])")
    scans = mvs_io.read_testlist(args.testlist)
    jobs = {folder: _folder_jobs(args.gtpath, args.outdir, scans, folder) for folder in args.folders}   # every file resolved first
    results: Dict[str, Dict[str, float]] = {}
    for folder in args.folders:
        r = score_files(jobs[folder], dev)
        results[folder] = r
        print(f"{folder}: " + "  ".join(f"{k} {r[k]:.4f}" for k in PRECISION_NAMES) + f"  ({r['images']} images)", flush=True)
    out = {"folders": results, "scans": scans}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
