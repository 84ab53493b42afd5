"""Training samples from DTU / BlendedMVS scenes on disk: the reference's ``datasets/dtu_yao.py`` and ``datasets/blended_dataset.py``
restated, with the per-pixel work on the GPU.

The reference prepares a sample on the host (``np.array(img, float32) / 255.``, crop, ``np.stack(...).transpose(0, 3, 1, 2)``, four
``cv2.resize`` per ground-truth map) and uploads float32.  Here a dataset's :meth:`load` only DECODES (PIL, ``mvs_io.read_pfm``) - uint8
pixels, the raw depth map, the raw mask png - and :class:`TrainBatches` uploads those bytes once per batch and runs
``ops.image_batch`` (crop + HWC -> CHW + ``/255``, csrc/train_data.hip) and ``ops.gt_pyramid`` (resize + crop + the four levels + mask,
csrc/depth_metrics.hip) on them.  cv2 is not installed in this project's environment: the restatement could not be compared with a
run of the reference's dataset modules; ``tests/train_data_ref.py`` restates them a second time in numpy / PIL for the tests.

Rules that parity depends on:

* DTU metas (dtu_yao.py:28-54): ONE ``Cameras/pair.txt`` serves all scans; one meta per scan x viewpoint x light 0..6, in that order.
  Images ``Rectified/{scan}_train/rect_{vid+1:03d}_{light}_r5000.png``, cameras ``Cameras/train/{vid:08d}_cam.txt``, ground truth
  ``Depths_raw/{scan}/depth_map_{vid:04d}.pfm`` and ``depth_visual_{vid:04d}.png``.  ``depth_interval = line11[1] * interval_scale``,
  ``depth_values = np.arange(dmin, interval * ndepths + dmin, interval, dtype=np.float32)`` in the same Python-float arithmetic, so the
  LENGTH is the reference's too (425 / 2.5 / 1.06: 192 values at ndepths = 192, but 49 at ndepths = 48).  Images are used at their stored
  size, uncropped; one whose size is not the ground-truth crop size raises.  Ground truth: the ``"dtu"`` layout of
  ``depth_eval.gt_tables`` (halve with INTER_NEAREST, centre crop 512 x 640, mask = png > 10).
* Blended metas (blended_dataset.py:21-50): each scan has its own ``{scan}/cams/pair.txt``; a viewpoint with no source view is dropped,
  one with fewer than ``nviews`` sources is padded with ``src_views[0]`` up to length ``nviews``.  Images
  ``{scan}/blended_images/{vid:08d}.jpg``, cameras ``{scan}/cams/{vid:08d}_cam.txt``, depth ``{scan}/rendered_depth_maps/{vid:08d}.pfm``.
  ``intrinsics[:2] /= 4``; with a third value n on line 11, ``interval = (dmin + int(float(n)) * interval - dmin) / ndepths``, then
  ``* interval_scale``; ``depth_values = np.arange(dmin, interval * (ndepths - 0.5) + dmin, interval, float32)``.  Image and ground truth
  are centre-cropped to 576 x 768 and the principal point is NOT moved by the crop: the reference leaves that line commented out
  (blended_dataset.py:63-64), and so does this module.
* ``proj[2,4,4]`` per view = (extrinsic, intrinsic in [:3,:3]); intrinsic rows 0-1 scaled x0.5 / x1 / x2 / x4 for stage1..stage4.
* View choice: ``val`` takes the first ``nviews - 1`` sources; ``train`` takes a permutation of the sources (Blended: of the first 7
  only) drawn from ``np.random.default_rng([seed, epoch, index])``.  The reference shuffles with the process-global numpy state inside
  forked workers - DTU even shuffles the stored meta in place - which no seed reproduces; this rule replaces it, and the stored metas
  are never modified.
* ``crop=(h, w)`` replaces the crop size of both layouts (as in ``depth_eval.read_gt_ms``).

:class:`TrainBatches` is one epoch of batches: decode ahead on a small thread pool into a ring of pinned staging buffers, upload and
prepare in order on the caller's stream.  No worker processes, no side stream (see its docstring).
"""
from __future__ import annotations

import os
import re
import threading
from concurrent.futures import Future, ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import mvs_io
from .depth_eval import DTU_MASK_THRESHOLD, LAYOUTS, gt_tables

Tensor = torch.Tensor

MAX_THREADS = 16                                              # hard cap of the decode pool, whatever the machine has
BLENDED_TRAIN_SOURCES = 7                                     # blended_dataset.py:129
DTU_LIGHTS = 7                                                # dtu_yao.py:50
STAGE_SCALES = (("stage1", 0.5), ("stage2", 1.0), ("stage3", 2.0), ("stage4", 4.0))


# ---------------------------------------------------------------------------------------------------------------------
# host readers
def _read_pairs(path: str) -> List[Tuple[int, List[int]]]:
    with open(path) as f:
        n = int(f.readline())
        out = []
        for _ in range(n):
            ref = int(f.readline().rstrip())
            out.append((ref, [int(x) for x in f.readline().rstrip().split()[1::2]]))
    return out


def _read_rgb(path: str) -> np.ndarray:
    """A decoded image as uint8 [H,W,3]; anything but 8-bit RGB raises (the reference would build a batch of another rank)."""
    from PIL import Image
    with Image.open(path) as img:
        if img.mode != "RGB":
            raise ValueError(f"{path}: expected an 8-bit RGB image, got mode {img.mode!r}")
        a = np.asarray(img)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"{path}: expected uint8 [H,W,3], got {a.dtype} {a.shape}")
    return a


def _image_size(path: str) -> Tuple[int, int]:
    from PIL import Image
    with Image.open(path) as img:                             # the header alone
        return int(img.size[1]), int(img.size[0])


def _pfm_size(path: str) -> Tuple[int, int]:
    with open(path, "rb") as f:
        f.readline()
        m = re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode("utf-8"))
    if not m:
        raise ValueError(f"{path}: malformed PFM header")
    return int(m.group(2)), int(m.group(1))


def _read_mask8(path: str) -> np.ndarray:
    """depth_visual png as uint8 [H,W]; an image of another depth is thresholded here (> 10 -> 255), as depth_eval does."""
    from PIL import Image
    with Image.open(path) as img:
        a = np.asarray(img)
    if a.ndim != 2:
        raise ValueError(f"{path}: expected a single-channel mask image, got shape {a.shape}")
    if a.dtype != np.uint8:
        a = np.where(a.astype(np.float64) > DTU_MASK_THRESHOLD, 255, 0).astype(np.uint8)
    return a


def stage_matrices(proj: np.ndarray) -> Dict[str, np.ndarray]:
    """proj [N,2,4,4] -> {stage1..stage4}: copies with intrinsic rows 0-1 x0.5 / x1 / x2 / x4 (dtu_yao.py:178-192)."""
    out = {}
    for name, s in STAGE_SCALES:
        m = proj.copy()
        if s != 1.0:
            m[:, 1, :2, :] = proj[:, 1, :2, :] * s
        out[name] = m
    return out


# ---------------------------------------------------------------------------------------------------------------------
# datasets
class _TrainScenes:
    layout = ""

    def __init__(self, datapath: str, listfile: str, mode: str, nviews: int, ndepths: int = 192, interval_scale: float = 1.06,
                 crop: Optional[Tuple[int, int]] = None, seed: int = 0):
        if mode not in ("train", "val"):
            raise ValueError(f"mode must be 'train' or 'val', got {mode!r}")
        if int(nviews) < 2:
            raise ValueError("nviews counts the reference view: at least 2")
        self.datapath, self.listfile, self.mode = str(datapath), str(listfile), mode
        self.nviews, self.ndepths, self.interval_scale, self.seed = int(nviews), int(ndepths), float(interval_scale), int(seed)
        self.crop = (int(crop[0]), int(crop[1])) if crop is not None else LAYOUTS[self.layout]["crop"]
        with open(self.listfile) as f:
            self.scans = [ln.rstrip() for ln in f if ln.strip()]
        self.metas: Tuple[tuple, ...] = tuple(self._build_list())      # tuples all the way down: nothing shuffles them in place
        self.tables: Dict[tuple, Tuple[Tensor, Tensor]] = {}           # device index tables, filled by TrainBatches, one per size
        self._sizes: Optional[Tuple[Tuple[int, int], Tuple[int, int]]] = None

    def __len__(self) -> int:
        return len(self.metas)

    # -- per layout ------------------------------------------------------------------------------------------------
    def _build_list(self) -> List[tuple]:
        raise NotImplementedError

    def _sources(self, index: int) -> Tuple[int, ...]:
        raise NotImplementedError

    def _paths(self, index: int, vid: int) -> Dict[str, str]:
        raise NotImplementedError

    def _read_cam(self, path: str) -> Tuple[np.ndarray, np.ndarray, float, float]:
        raise NotImplementedError

    def _depth_values(self, dmin: float, interval: float) -> np.ndarray:
        raise NotImplementedError

    def _name(self, index: int, ref: int) -> str:
        return self.metas[index][0] + "/{}/" + "{:0>8}".format(ref) + "{}"     # blended_dataset.py:188

    # -- shared ----------------------------------------------------------------------------------------------------
    def view_ids(self, index: int, epoch: int = 0) -> List[int]:
        """[reference view, nviews - 1 sources]: the first sources in ``val`` mode, a permutation that depends on (seed, epoch, index)
        alone in ``train`` mode."""
        ref = self._ref(index)
        src = list(self._sources(index))
        if self.mode == "train":
            perm = np.random.default_rng([self.seed, int(epoch), int(index)]).permutation(len(src))
            src = [src[i] for i in perm]
        return [ref] + src[:self.nviews - 1]

    def _ref(self, index: int) -> int:
        raise NotImplementedError

    def files(self, index: int, epoch: int = 0) -> List[str]:
        """Every file :meth:`load` will open for this sample."""
        out: List[str] = []
        for i, vid in enumerate(self.view_ids(index, epoch)):
            p = self._paths(index, vid)
            out += [p["img"], p["cam"]] + ([p["depth"]] + ([p["mask"]] if "mask" in p else []) if i == 0 else [])
        return out

    def sizes(self) -> Tuple[Tuple[int, int], Tuple[int, int]]:
        """((image rows, cols), (ground-truth rows, cols)) as stored, from the headers of the first meta's reference view; every other
        file must agree (:meth:`load` checks)."""
        if self._sizes is None:
            if not self.metas:
                raise ValueError(f"{self.listfile}: no training views")
            p = self._paths(0, self._ref(0))
            self._sizes = (_image_size(p["img"]), _pfm_size(p["depth"]))
        return self._sizes

    def image_tables(self, Hs: int, Ws: int) -> Tuple[np.ndarray, np.ndarray]:
        """(rows, cols) of ``ops.image_batch`` for an Hs x Ws image."""
        raise NotImplementedError

    def load(self, index: int, epoch: int = 0, out: Optional[Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]] = None) -> Dict[str, object]:
        """Decode one sample on the host - no GPU call, safe on a thread.  -> {"imgs": uint8 [N,Hs,Ws,3], "depth": the raw float32 depth
        map [Hg,Wg], "mask8": the raw uint8 mask png [Hg,Wg] (DTU; None for Blended), "proj": float32 [N,2,4,4], "depth_values": float32
        [D], "filename", "view_ids"}.  ``out`` = (imgs, depth, mask8) arrays of those shapes to decode into (staging memory)."""
        ids = self.view_ids(index, epoch)
        imgs = out[0] if out is not None else None
        proj = np.zeros((len(ids), 2, 4, 4), np.float32)
        depth = mask8 = dv = None
        for i, vid in enumerate(ids):
            p = self._paths(index, vid)
            a = _read_rgb(p["img"])
            if imgs is None:
                imgs = np.empty((len(ids),) + a.shape, np.uint8)
            if a.shape != imgs.shape[1:]:
                raise ValueError(f"{p['img']}: image is {a.shape[0]} x {a.shape[1]}, expected {imgs.shape[1]} x {imgs.shape[2]} "
                                 "(all views of a dataset must have one size)")
            np.copyto(imgs[i], a)
            try:
                intr, extr, dmin, interval = self._read_cam(p["cam"])
            except (IndexError, ValueError) as e:
                raise ValueError(f"{p['cam']}: malformed camera file ({e})") from e
            proj[i, 0] = extr
            proj[i, 1, :3, :3] = intr
            if i == 0:
                d = mvs_io.read_pfm(p["depth"])[0]
                if d.ndim != 2:
                    raise ValueError(f"{p['depth']}: expected a single-channel depth map")
                if out is not None:
                    if d.shape != out[1].shape:
                        raise ValueError(f"{p['depth']}: depth map is {d.shape}, expected {out[1].shape}")
                    np.copyto(out[1], d)
                    d = out[1]
                depth = d
                if "mask" in p:
                    m = _read_mask8(p["mask"])
                    if m.shape != d.shape:
                        raise ValueError(f"{p['mask']}: mask is {m.shape}, the depth map {d.shape}")
                    if out is not None:
                        np.copyto(out[2], m)
                        m = out[2]
                    mask8 = m
                dv = self._depth_values(dmin, interval)
        return {"imgs": imgs, "depth": depth, "mask8": mask8, "proj": proj, "depth_values": dv,
                "filename": self._name(index, ids[0]), "view_ids": ids}


def _cam_lines(path: str) -> List[str]:
    with open(path) as f:
        return [ln.rstrip() for ln in f.readlines()]


def _cam_matrices(lines: List[str]) -> Tuple[np.ndarray, np.ndarray]:
    extr = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape(4, 4)
    intr = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape(3, 3)
    return intr, extr


class DTUTrainScenes(_TrainScenes):
    """``datasets/dtu_yao.py`` (the DTU training set as preprocessed for MVSNet); see the module docstring."""
    layout = "dtu"

    def _build_list(self):
        metas = []
        for scan in self.scans:
            for ref, src in _read_pairs(os.path.join(self.datapath, "Cameras/pair.txt")):
                for light in range(DTU_LIGHTS):
                    metas.append((scan, light, ref, tuple(src)))
        return metas

    def _ref(self, index):
        return self.metas[index][2]

    def _sources(self, index):
        return self.metas[index][3]

    def _paths(self, index, vid):
        scan, light = self.metas[index][0], self.metas[index][1]
        return {"img": os.path.join(self.datapath, "Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, vid + 1, light)),
                "cam": os.path.join(self.datapath, "Cameras/train/{:0>8}_cam.txt".format(vid)),
                "depth": os.path.join(self.datapath, "Depths_raw/{}/depth_map_{:0>4}.pfm".format(scan, vid)),
                "mask": os.path.join(self.datapath, "Depths_raw/{}/depth_visual_{:0>4}.png".format(scan, vid))}

    def _read_cam(self, path):
        lines = _cam_lines(path)
        intr, extr = _cam_matrices(lines)
        f = lines[11].split()
        return intr, extr, float(f[0]), float(f[1]) * self.interval_scale

    def _depth_values(self, dmin, interval):
        return np.arange(dmin, interval * self.ndepths + dmin, interval, dtype=np.float32)

    def image_tables(self, Hs, Ws):
        if (Hs, Ws) != self.crop:
            raise ValueError(f"DTU training images are used as stored: a {Hs} x {Ws} image does not match the "
                             f"{self.crop[0]} x {self.crop[1]} ground-truth crop")
        return np.arange(Hs, dtype=np.int64), np.arange(Ws, dtype=np.int64)


class BlendedTrainScenes(_TrainScenes):
    """``datasets/blended_dataset.py`` (BlendedMVS, low resolution); see the module docstring."""
    layout = "blended"

    def _build_list(self):
        metas = []
        for scan in self.scans:
            for ref, src in _read_pairs(os.path.join(self.datapath, "{}/cams/pair.txt".format(scan))):
                if len(src) > 0:
                    if len(src) < self.nviews:
                        src = src + [src[0]] * (self.nviews - len(src))
                    metas.append((scan, ref, tuple(src)))
        return metas

    def _ref(self, index):
        return self.metas[index][1]

    def _sources(self, index):
        src = self.metas[index][2]
        return src[:BLENDED_TRAIN_SOURCES] if self.mode == "train" else src

    def _paths(self, index, vid):
        scan = self.metas[index][0]
        return {"img": os.path.join(self.datapath, "{}/blended_images/{:0>8}.jpg".format(scan, vid)),
                "cam": os.path.join(self.datapath, "{}/cams/{:0>8}_cam.txt".format(scan, vid)),
                "depth": os.path.join(self.datapath, "{}/rendered_depth_maps/{:0>8}.pfm".format(scan, vid))}

    def _read_cam(self, path):
        lines = _cam_lines(path)
        intr, extr = _cam_matrices(lines)
        intr[:2, :] /= 4.0
        f = lines[11].split()
        dmin, interval = float(f[0]), float(f[1])
        if len(f) >= 3:
            dmax = dmin + int(float(f[2])) * interval
            interval = (dmax - dmin) / self.ndepths
        return intr, extr, dmin, interval * self.interval_scale

    def _depth_values(self, dmin, interval):
        return np.arange(dmin, interval * (self.ndepths - 0.5) + dmin, interval, dtype=np.float32)

    def image_tables(self, Hs, Ws):
        return gt_tables(Hs, Ws, "blended", self.crop)        # the same centre crop as the ground truth (blended_dataset.py:79-92)


# ---------------------------------------------------------------------------------------------------------------------
# one epoch's order
def epoch_batches(n: int, batch_size: int, seed: int = 0, epoch: int = 0, shuffle: bool = True, drop_last: bool = True,
                  rank: int = 0, world: int = 1) -> List[List[int]]:
    """The batches of sample indices rank ``rank`` of ``world`` sees in ``epoch``: a permutation from
    ``np.random.default_rng([seed, epoch])`` when shuffling, cut into batches (a short last one dropped with ``drop_last``); rank r takes
    batches r::world of the leading ``len - len % world``, so every rank gets the same number."""
    n, batch_size, rank, world = int(n), int(batch_size), int(rank), int(world)
    if batch_size < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"epoch_batches: batch_size {batch_size}, rank {rank} of {world}")
    order = np.random.default_rng([int(seed), int(epoch)]).permutation(n) if shuffle else np.arange(n)
    batches = [[int(i) for i in order[s:s + batch_size]] for s in range(0, n, batch_size)]
    if drop_last and batches and len(batches[-1]) < batch_size:
        batches.pop()
    keep = len(batches) - len(batches) % world
    return batches[:keep][rank::world]


def _align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


class DecodeAhead:
    """What :class:`TrainBatches` and ``eval_data.EvalViews`` share: the decode pool, the ring of staging-buffer events and the
    iterator's life cycle - ONE copy of the rules that keep a staging buffer from being refilled while a copy still reads it.

    ``_start(fn, *args)`` runs one decode, on the pool (created on first use: ``threads`` workers, at most 16, never sized from the
    machine's CPU count) or, with ``ahead=0``, at once on the caller's thread; either way the result or the exception is in the
    returned future.  ``_record(s)`` marks, on the caller's current stream, the end of the copy that reads staging buffer ``s``;
    ``_wait(s)`` makes the host wait for it, and must precede every refill of that buffer.  ``close()``, exhaustion, an exception and
    ``__del__`` shut the pool down; a worker never waits on a queue, so none can be left blocked.  A subclass keeps its scheduled
    work in ``self._pending`` and says in ``_futures`` which futures that holds."""

    def __init__(self, threads: int, ahead: int, name: str):
        self.ahead, self.threads = int(ahead), int(threads)
        if self.ahead < 0 or not 1 <= self.threads <= MAX_THREADS:
            raise ValueError(f"{type(self).__name__}: ahead must be >= 0 and threads 1..{MAX_THREADS}, got {ahead}, {threads}")
        self._pool_name = name
        self._pool: Optional[ThreadPoolExecutor] = None
        self._events: List[Optional["torch.cuda.Event"]] = [None] * (self.ahead + 1)
        self._pending: Dict[int, object] = {}
        self._scheduled = 0
        self._k = 0
        self._closed = False
        self._lock = threading.Lock()

    def __iter__(self):
        return self

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> bool:
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:                                     # interpreter shutdown
            pass

    def _futures(self, pending) -> List[Future]:
        raise NotImplementedError

    def close(self) -> None:
        """Drop what has not started, wait for the (finite) decodes that have, join the workers.  Idempotent."""
        with self._lock:
            self._closed = True
            pool, self._pool = self._pool, None
            pending, self._pending = self._pending, {}
        for f in self._futures(pending):
            f.cancel()
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)

    def _start(self, fn, *args) -> Future:
        if self.ahead > 0:
            if self._pool is None:
                self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix=self._pool_name)
            return self._pool.submit(fn, *args)
        f: Future = Future()
        try:
            f.set_result(fn(*args))
        except Exception as e:
            f.set_exception(e)
        return f

    def _wait(self, s: int) -> None:
        ev = self._events[s]
        if ev is not None:                                    # the copy that last read this buffer must have finished
            ev.synchronize()
            self._events[s] = None

    def _record(self, s: int) -> None:
        ev = torch.cuda.Event()
        ev.record()
        self._events[s] = ev


class TrainBatches(DecodeAhead):
    """One epoch of ``train.train_step`` samples from a :class:`DTUTrainScenes` / :class:`BlendedTrainScenes`, an iterator.

    Order: :func:`epoch_batches` (``shuffle`` and ``drop_last`` default to the dataset's train mode, as in the reference's loaders).

    Decode ahead: up to ``ahead`` batches beyond the one being consumed are decoded by a ``ThreadPoolExecutor`` of ``threads`` workers
    (default 4, never more than 16, never sized from the machine's CPU count), one ``dataset.load`` per task, straight into a ring of
    ``ahead + 1`` pinned staging buffers (per buffer: the batch's uint8 images, then the raw ground-truth depth maps, then the raw mask
    pngs).  Threads, not processes: PIL's decoders release the GIL, a forked child of a process that has opened the GPU is a known way
    to hang, and a thread needs no GPU context.  ``ahead=0`` runs the same code with no pool, each batch decoded when it is asked for.

    In-order upload: ``__next__`` runs on the caller's thread and the caller's current stream: ONE ``non_blocking`` copy of the staged
    bytes, an event, ``ops.image_batch`` for the whole batch, ``ops.gt_pyramid`` per sample, a stack per stage.  A staging buffer goes
    back to the decoders only after its event has completed (the host waits for it when it schedules the batch that reuses the
    buffer - by then the copy is one step old).  No side stream and no ``record_stream``: in-order issue has no cross-stream allocator
    hazard, and the upload is small next to a step.

    Files are checked to exist when a batch is scheduled, on the caller's thread and before any device call, so a missing file fails
    fast with its path.  An exception in a worker is re-raised by ``__next__`` (its message carries the file name).  ``close()``,
    exhaustion, an exception and ``__del__`` all shut the pool down; a worker never waits on a queue, so none can be left blocked.

    Yields {"imgs" [B,N,3,H,W], "depth" / "mask" {stageK: [B,h,w]}} on ``device`` and {"proj_matrices" {stageK: [B,N,2,4,4]},
    "depth_values" [B,D]} on the HOST, where ``training.train_geometry`` wants them (it would read device tensors back), plus
    "filename" (a list)."""

    def __init__(self, dataset: _TrainScenes, batch_size: int, device, epoch: int = 0, shuffle: Optional[bool] = None,
                 drop_last: Optional[bool] = None, rank: int = 0, world: int = 1, threads: int = 4, ahead: int = 2):
        self.dataset, self.batch_size, self.epoch = dataset, int(batch_size), int(epoch)
        self.device = torch.device(device)
        train = dataset.mode == "train"
        self.batches = epoch_batches(len(dataset), self.batch_size, dataset.seed, self.epoch, train if shuffle is None else bool(shuffle),
                                     train if drop_last is None else bool(drop_last), rank, world)
        super().__init__(threads, ahead, "cds-decode")
        self._ring: List[Optional[dict]] = [None] * (self.ahead + 1)

    def __len__(self) -> int:
        return len(self.batches)

    def _futures(self, pending) -> List[Future]:
        return [f for futs in pending.values() for f in futs]

    # -- staging ---------------------------------------------------------------------------------------------------
    def _slot(self, s: int) -> dict:
        """Staging buffer s: one pinned byte tensor and numpy views of its three sections."""
        slot = self._ring[s]
        if slot is None:
            ds = self.dataset
            (Hs, Ws), (Hg, Wg) = ds.sizes()
            N, Bmax = ds.nviews, self.batch_size
            n_img, n_gt = Bmax * N * Hs * Ws * 3, Bmax * Hg * Wg
            off_d = _align(n_img)
            off_m = _align(off_d + 4 * n_gt)
            total = off_m + (n_gt if ds.layout == "dtu" else 0)
            buf = torch.empty(total, dtype=torch.uint8).pin_memory()
            host = buf.numpy()
            slot = self._ring[s] = {
                "buf": buf, "off_d": off_d, "off_m": off_m, "sizes": (Hs, Ws, Hg, Wg),
                "imgs": host[:n_img].reshape(Bmax, N, Hs, Ws, 3),
                "depth": host[off_d:off_d + 4 * n_gt].view(np.float32).reshape(Bmax, Hg, Wg),
                "mask": host[off_m:off_m + n_gt].reshape(Bmax, Hg, Wg) if ds.layout == "dtu" else None}
        return slot

    def _schedule(self, upto: int) -> None:
        """Start the decodes of batches < upto that have not been started."""
        while self._scheduled < min(upto, len(self.batches)):
            j = self._scheduled
            idx = self.batches[j]
            for i in idx:                                     # fail fast, on the caller's thread, before any device call
                for path in self.dataset.files(i, self.epoch):
                    if not os.path.isfile(path):
                        raise FileNotFoundError(f"{path}: not found (sample {i} of {self.dataset.listfile})")
            s = j % (self.ahead + 1)
            self._wait(s)
            slot = self._slot(s)
            futs = []
            for b, i in enumerate(idx):
                out = (slot["imgs"][b], slot["depth"][b], slot["mask"][b] if slot["mask"] is not None else None)
                futs.append(self._start(self.dataset.load, i, self.epoch, out))
            self._pending[j] = futs
            self._scheduled += 1

    def _tables(self, kind: str, Hs: int, Ws: int) -> Tuple[Tensor, Tensor]:
        from . import ops
        ds = self.dataset
        key = (kind, Hs, Ws, ds.crop, str(self.device))
        if key not in ds.tables:                              # one upload per dataset and source size
            host = ds.image_tables(Hs, Ws) if kind == "img" else gt_tables(Hs, Ws, ds.layout, ds.crop)
            ds.tables[key] = ops.index_tables(host[0], host[1], Hs, Ws, self.device)
        return ds.tables[key]

    def __next__(self) -> Dict[str, object]:
        from . import ops
        if self._closed or self._k >= len(self.batches):
            self.close()
            raise StopIteration
        k = self._k
        try:
            self._schedule(k + self.ahead + 1)
            recs = [f.result() for f in self._pending.pop(k)]
            B = len(recs)
            slot = self._ring[k % (self.ahead + 1)]
            Hs, Ws, Hg, Wg = slot["sizes"]
            N = self.dataset.nviews
            dev = self.device
            with torch.cuda.device(dev):
                img_tab = self._tables("img", Hs, Ws)
                gt_tab = self._tables("gt", Hg, Wg)
                staged = slot["buf"].to(dev, non_blocking=True)             # the one copy, on the current stream
                self._record(k % (self.ahead + 1))
                n_img, n_gt = self.batch_size * N * Hs * Ws * 3, self.batch_size * Hg * Wg
                u8 = staged[:n_img].view(self.batch_size * N, Hs, Ws, 3)[:B * N]
                imgs = ops.image_batch(u8, img_tab[0], img_tab[1])
                imgs = imgs.view(B, N, 3, imgs.shape[2], imgs.shape[3])
                dsrc = staged[slot["off_d"]:slot["off_d"] + 4 * n_gt].view(torch.float32).view(self.batch_size, Hg, Wg)
                msrc = staged[slot["off_m"]:slot["off_m"] + n_gt].view(self.batch_size, Hg, Wg) if slot["mask"] is not None else None
                depths, masks = [], []
                for b in range(B):
                    d, m = ops.gt_pyramid(dsrc[b], gt_tab[0], gt_tab[1], levels=4, mask_src=msrc[b] if msrc is not None else None,
                                          mask_thresh=DTU_MASK_THRESHOLD)
                    depths.append(d)
                    masks.append(m)
                names = ["stage4", "stage3", "stage2", "stage1"]                # gt_pyramid: finest first
                depth = {nm: torch.stack([depths[b][lv] for b in range(B)]) for lv, nm in enumerate(names)}
                mask = {nm: torch.stack([masks[b][lv] for b in range(B)]) for lv, nm in enumerate(names)}
            proj = [stage_matrices(r["proj"]) for r in recs]
            lens = {len(r["depth_values"]) for r in recs}
            if len(lens) != 1:
                raise ValueError(f"{recs[0]['filename']}: the samples of a batch have {sorted(lens)} depth values; they must agree")
            self._k += 1
            return {"imgs": imgs,
                    "proj_matrices": {nm: torch.from_numpy(np.stack([p[nm] for p in proj])) for nm, _ in STAGE_SCALES},
                    "depth_values": torch.from_numpy(np.stack([r["depth_values"] for r in recs])),
                    "depth": depth, "mask": mask, "filename": [r["filename"] for r in recs]}
        except BaseException:
            self.close()
            raise
