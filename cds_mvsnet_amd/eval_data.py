"""Evaluation views prepared on the GPU and depth-map outputs packed on the GPU: what ``infer --pipeline gpu`` runs around the model
(the evaluation-side counterpart of ``train_data.TrainBatches``).

The host pipeline (``mvs_io.EvalScenes`` + ``mvs_io.save_outputs``) decodes N JPEGs per reference view, converts, resizes and uploads
float32, then reads five tensors back one by one and writes the files before the next forward may start.  Here

* :class:`EvalViews` decodes a view ONCE per scan (a DTU view is a source of about ten others): the uint8 pixels go through a pinned
  staging buffer to the device, ``ops.eval_views`` (csrc/eval_data.hip) makes the ``[3, max_h, max_w]`` float32 view - ``/255``, the
  Tanks & Temples edge padding, the resize, HWC -> CHW - and a byte-bounded LRU cache keeps it for the reference views that follow.
* :class:`OutputWriter` packs a depth map's side outputs with ``ops.eval_outputs``, copies them to pinned memory without blocking
  the host and writes the files on one thread while the next forward runs.

Resize rule.  An image that is not ``max_h x max_w`` (after the padding) is resized as the reference resizes it:
``cv2.resize(float32 image, (max_w, max_h), interpolation=cv2.INTER_LINEAR)`` (datasets/general_eval.py:100-118), plain bilinear with
no antialiasing, restated in :func:`linear_tables` and the kernel.  ``EvalScenes`` quantises to uint8 and calls PIL ``BILINEAR``, an
antialiasing filter when it shrinks: the two pipelines give DIFFERENT pixels for such images, and the same pixels (``u8 / 255``
exactly) for images that need no resize.  cv2 is not installed in this project's environment: the rule is restated from OpenCV's
source and the tests compare against a second numpy restatement (tests/eval_data_ref.py), not against a run of cv2.  Rows use the
x rule; OpenCV itself keeps ``fy`` on a clamped row, which differs by at most 1 ulp and only in top / bottom rows that are enlarged
(DESIGN.md §1.5).

Cameras: the metas and the source-view padding are ``EvalScenes``'s own (an instance is held for them), the camera files are read by
``mvs_io.read_cam_file``; :meth:`EvalViews._camera` / :meth:`EvalViews._stages` follow ``EvalScenes.__getitem__`` line by line (that
method interleaves them with the image work and cannot be called without it) and the tests hold the two equal.
"""
from __future__ import annotations

import os
import queue
import threading
from collections import OrderedDict
from concurrent.futures import Future
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import mvs_io
from .train_data import DecodeAhead, _align, _image_size

Tensor = torch.Tensor

TT_PAD = 4                                                    # Tanks & Temples: 1080 -> 1088 rows (general_eval.py:92-93)


# ---------------------------------------------------------------------------------------------------------------------
# tables
def linear_tables(S: int, d: int, pad: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The taps of OpenCV's float32 INTER_LINEAR along one axis: a source of S samples, edge-padded by ``pad`` on both sides, resized
    to d samples -> (s0 int32 [d], s1 int32 [d], f float32 [d]): ``out = src[s0] * (1 - f) + src[s1] * f``.

    ``scale = 1.0 / (d / Sp)`` in double (Sp = S + 2 pad), ``f = float32((x + 0.5) * scale - 0.5)``, ``s = floor(f)``, ``f -= s``;
    ``s < 0`` -> ``s = 0, f = 0``; ``s >= Sp - 1`` -> ``s = Sp - 1, f = 0``; the second tap is ``min(s + 1, Sp - 1)``.  The padding
    is folded in last: both taps become ``clip(tap - pad, 0, S - 1)``, so no padded copy is needed.  Sp == d gives s = arange, f = 0."""
    S, d, pad = int(S), int(d), int(pad)
    if S < 1 or d < 1 or pad < 0:
        raise ValueError(f"linear_tables: source {S}, target {d}, pad {pad}")
    Sp = S + 2 * pad
    scale = 1.0 / (d / Sp)
    f = ((np.arange(d, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= Sp - 1
    s = np.where(lo, 0, np.where(hi, Sp - 1, s))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    s1 = np.minimum(s + 1, Sp - 1)
    return (np.clip(s - pad, 0, S - 1).astype(np.int32), np.clip(s1 - pad, 0, S - 1).astype(np.int32), f)


def nearest_tables(S: int, d: int) -> np.ndarray:
    """``mvs_io.nearest_resize``'s source index of each of d output samples: ``min(int(i * (S / d)), S - 1)``, S / d in double."""
    return np.minimum((np.arange(int(d)) * (int(S) / int(d))).astype(np.int64), int(S) - 1).astype(np.int32)


_TABLES: Dict[tuple, tuple] = {}
_TABLES_LOCK = threading.Lock()


def _upload(ints: np.ndarray, floats: Optional[np.ndarray], device) -> Tuple[Tensor, Optional[Tensor]]:
    """BLOCKING copies: the tables are cached for the life of the process and used from whatever stream a later caller is on, so they
    must be on the device when this returns (a few KB, once per shape)."""
    ti = torch.from_numpy(np.ascontiguousarray(ints, dtype=np.int32)).to(device)
    tf = torch.from_numpy(np.ascontiguousarray(floats, dtype=np.float32)).to(device) if floats is not None else None
    return ti, tf


def view_tables(Hs: int, Ws: int, pad: int, h: int, w: int, device) -> Tuple[Tuple[Tensor, Tensor, Tensor], Tuple[Tensor, Tensor, Tensor]]:
    """(rows, cols) of ``ops.eval_views`` for Hs x Ws views, ``pad`` edge rows above and below, resized to h x w: built once per
    (Hs, Ws, pad, h, w, device), uploaded once, cached for the life of the process (a few KB each)."""
    device = torch.device(device)
    key = ("view", int(Hs), int(Ws), int(pad), int(h), int(w), str(device))
    with _TABLES_LOCK:
        if key not in _TABLES:
            r0, r1, fy = linear_tables(Hs, h, pad)
            c0, c1, fx = linear_tables(Ws, w, 0)
            ti, tf = _upload(np.concatenate((r0, r1, c0, c1)), np.concatenate((fy, fx)), device)
            h, w = int(h), int(w)
            _TABLES[key] = ((ti[:h], ti[h:2 * h], tf[:h]), (ti[2 * h:2 * h + w], ti[2 * h + w:], tf[h:]))
        return _TABLES[key]


def output_tables(shapes: Sequence[Tuple[int, int]], h: int, w: int, device) -> Tensor:
    """The ``tab`` of ``ops.eval_outputs``: shapes = the (rows, cols) of conf1, conf2, conf3 and the image; int32 [4 h + 4 w] on the
    device - source rows of the four for each output row, then source columns.  Cached like :func:`view_tables`."""
    device = torch.device(device)
    shapes = tuple((int(a), int(b)) for a, b in shapes)
    if len(shapes) != 4:
        raise ValueError("output_tables: shapes of conf1, conf2, conf3 and the image")
    key = ("out", shapes, int(h), int(w), str(device))
    with _TABLES_LOCK:
        if key not in _TABLES:
            tab = np.concatenate([nearest_tables(a, h) for a, _ in shapes] + [nearest_tables(b, w) for _, b in shapes])
            _TABLES[key] = _upload(tab, None, device)[0]
        return _TABLES[key]


# ---------------------------------------------------------------------------------------------------------------------
# the per-view cache
class ViewCache:
    """Least-recently-used cache bounded in BYTES.  ``get`` counts a hit and refreshes the entry; ``put`` counts a decode, inserts, and
    evicts from the cold end while the total exceeds the capacity - the entry just inserted included, when it alone is larger than
    the capacity: the caller holds its own reference, so such a view is served once and not kept.  Values are opaque (device
    tensors in :class:`EvalViews`, anything in a test); not thread-safe, it lives on the caller's thread."""

    def __init__(self, capacity_bytes: int):
        self.capacity = int(capacity_bytes)
        if self.capacity < 0:
            raise ValueError("ViewCache: capacity must be >= 0")
        self.bytes = 0
        self.stats: Dict[str, int] = {"decodes": 0, "hits": 0, "evictions": 0}
        self._d: "OrderedDict[object, Tuple[object, int]]" = OrderedDict()

    def __len__(self) -> int:
        return len(self._d)

    def __contains__(self, key) -> bool:
        return key in self._d

    def keys(self) -> List[object]:
        return list(self._d)

    def get(self, key):
        e = self._d.get(key)
        if e is None:
            return None
        self._d.move_to_end(key)
        self.stats["hits"] += 1
        return e[0]

    def put(self, key, value, nbytes: int) -> None:
        self.stats["decodes"] += 1
        old = self._d.pop(key, None)
        if old is not None:
            self.bytes -= old[1]
        self._d[key] = (value, int(nbytes))
        self.bytes += int(nbytes)
        while self.bytes > self.capacity and self._d:
            _, (_, n) = self._d.popitem(last=False)
            self.bytes -= n
            self.stats["evictions"] += 1


# ---------------------------------------------------------------------------------------------------------------------
# views
def _decode(path: str, dst: np.ndarray) -> None:
    """One view as PIL decodes it (``convert("RGB")``, as EvalScenes) into staging memory.  Host only: safe on a thread."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"))
    if a.shape != dst.shape:
        raise ValueError(f"{path}: decoded to {a.shape}, its header said {dst.shape}")
    np.copyto(dst, a)


class EvalViews(DecodeAhead):
    """The samples of ``mvs_io.EvalScenes`` with the images prepared on the GPU, an iterator.

    Constructor fields are EvalScenes's, plus ``device``, ``cache_mb`` (the per-view cache, in MiB of prepared float32 views),
    ``threads`` / ``ahead`` (the decode pool and how many samples beyond the current one it works on; ``ahead=0``: no pool) and
    ``rank`` / ``world`` (this rank takes the metas ``idx % world == rank``, as ``infer`` shards them) or ``indices`` (which metas, in
    which order).

    Yields {"imgs": [1, N, 3, max_h, max_w] float32 on ``device``, "proj_matrices" {stageK: numpy [N,2,4,4]}, "depth_values": numpy
    [D], "filename"} - everything but ``imgs`` exactly as ``EvalScenes.__getitem__`` returns it, on the host, where the model wants it.

    Cache: prepared views keyed by (scan, view id), LRU, bounded by ``cache_mb``; ``stats`` counts ``decodes``, ``hits`` and
    ``evictions``.  A view is looked up when its sample is SCHEDULED: a hit is held by the sample from then on (an eviction in between
    cannot take it away), a view that an earlier scheduled sample is already decoding is borrowed from that sample (counted as a
    hit), anything else is decoded for this sample.  All of a sample's missing views of one source size are prepared by ONE
    ``ops.eval_views`` launch; each prepared view owns its memory, so an eviction frees exactly the bytes the cache accounts for.

    Staging and stream order are ``TrainBatches``'s, through the shared ``train_data.DecodeAhead``: ``ahead + 1`` pinned byte buffers, decoders write straight into
    them, ``__next__`` issues one ``non_blocking`` copy of the used bytes on the caller's current stream and records an event; a
    buffer returns to the decoders only after its event has completed.  No worker processes, no side stream.  Every file of a sample
    is checked when the sample is scheduled, on the caller's thread and before any device call; a worker's exception is re-raised by
    ``__next__``; ``close()``, exhaustion and an exception shut the pool down."""

    def __init__(self, root: str, scans: Sequence[str], nviews: int = 5, ndepths: int = 192, interval_scale: float = 1.06,
                 max_h: int = 512, max_w: int = 640, refine: bool = False, dataset: str = "dtu", device="cuda", cache_mb: float = 2048,
                 threads: int = 4, ahead: int = 2, rank: int = 0, world: int = 1, indices: Optional[Iterable[int]] = None):
        super().__init__(threads, ahead, "cds-eval-decode")
        self.scenes = mvs_io.EvalScenes(root, scans, nviews=nviews, ndepths=ndepths, interval_scale=interval_scale, max_h=max_h,
                                        max_w=max_w, refine=refine, dataset=dataset)
        self.device = torch.device(device)
        if int(world) < 1 or not 0 <= int(rank) < int(world):
            raise ValueError(f"EvalViews: rank {rank} of {world}")
        self.order = list(range(int(rank), len(self.scenes), int(world))) if indices is None else [int(i) for i in indices]
        self.pad = TT_PAD if dataset == "tt" else 0
        self.cache = ViewCache(int(float(cache_mb) * (1 << 20)))
        self.stats = self.cache.stats
        self.view_bytes = 3 * int(max_h) * int(max_w) * 4
        self._paths: Dict[tuple, Tuple[str, int, int]] = {}            # (scan, vid) -> (image file, rows, cols as stored)
        self._cams: Dict[tuple, Tuple[np.ndarray, float, float]] = {}
        self._ring: List[Optional[Tensor]] = [None] * (self.ahead + 1)
        self._inflight: Dict[tuple, int] = {}                          # view -> the scheduled sample that decodes it
        self._ready: Dict[tuple, Tensor] = {}                          # prepared views a later scheduled sample borrows

    def __len__(self) -> int:
        return len(self.order)

    def _futures(self, pending) -> List[Future]:
        return [f for rec in pending.values() for f in rec["futs"]]

    def close(self) -> None:
        super().close()
        self._ready.clear()

    # -- files and cameras -----------------------------------------------------------------------------------------
    def _view(self, scan: str, vid: int) -> Tuple[str, int, int]:
        key = (scan, vid)
        if key not in self._paths:
            tried = [os.path.join(self.scenes.root, scan, sub, f"{vid:08d}.jpg") for sub in ("images_post", "images")]
            path = next((p for p in tried if os.path.isfile(p)), None)
            if path is None:
                raise FileNotFoundError(f"{tried[-1]}: not found (view {vid} of scan {scan})")
            self._paths[key] = (path,) + _image_size(path)
        return self._paths[key]

    def _cam_path(self, scan: str, vid: int) -> str:
        return os.path.join(self.scenes.root, scan, "cams", f"{vid:08d}_cam.txt")

    def _camera(self, scan: str, vid: int) -> Tuple[np.ndarray, float, float]:
        """One view's [2,4,4] matrix at stage-1 scale, depth_min, depth_interval: EvalScenes.__getitem__'s camera lines."""
        key = (scan, vid)
        if key not in self._cams:
            sc = self.scenes
            intr, extr, dmin, dint = mvs_io.read_cam_file(self._cam_path(scan, vid), sc.ndepths, sc.interval_scale)
            if sc.dataset == "tt":
                intr[1, 2] += 4
            intr[:2, :] /= 4.0
            _, Hs, Ws = self._view(scan, vid)
            h, w = Hs + 2 * self.pad, Ws
            if (h, w) != (sc.max_h, sc.max_w):
                intr[0, :] *= sc.max_w / w
                intr[1, :] *= sc.max_h / h
            m = np.zeros((2, 4, 4), dtype=np.float32)
            m[0] = extr
            m[1, :3, :3] = intr
            self._cams[key] = (m, dmin, dint)
        return self._cams[key]

    def _stages(self, base: np.ndarray) -> Dict[str, np.ndarray]:
        def scaled(f):
            m = base.copy()
            m[:, 1, :2, :] = base[:, 1, :2, :] * f
            return m
        if self.scenes.refine:
            return {"stage1": scaled(0.5), "stage2": base, "stage3": scaled(2), "stage4": scaled(4)}
        return {"stage1": base, "stage2": scaled(2), "stage3": scaled(4)}

    # -- decode ahead ----------------------------------------------------------------------------------------------
    def _schedule(self, upto: int) -> None:
        """Start the decodes of samples < upto that have not been started."""
        while self._scheduled < min(upto, len(self.order)):
            j = self._scheduled
            scan, ref, srcs = self.scenes.metas[self.order[j]]
            vids = [ref] + list(srcs)
            have: Dict[tuple, Tensor] = {}
            borrow: List[tuple] = []
            decode: List[tuple] = []
            for vid in dict.fromkeys(vids):                   # fail fast, on the caller's thread, before any device call
                cam = self._cam_path(scan, vid)
                if not os.path.isfile(cam):
                    raise FileNotFoundError(f"{cam}: not found (view {vid} of scan {scan})")
                path, Hs, Ws = self._view(scan, vid)
                key = (scan, vid)
                t = self.cache.get(key)
                if t is not None:
                    have[key] = t
                elif key in self._inflight:
                    borrow.append(key)
                    self.stats["hits"] += 1
                else:
                    decode.append((key, path, Hs, Ws))
            s = j % (self.ahead + 1)
            groups: Dict[Tuple[int, int], List[tuple]] = {}
            for item in decode:
                groups.setdefault((item[2], item[3]), []).append(item)
            layout, used = [], 0                               # [(Hs, Ws, offset, [keys])]: one eval_views launch each
            for (Hs, Ws), items in groups.items():
                layout.append((Hs, Ws, used, [it[0] for it in items], [it[1] for it in items]))
                used = _align(used + len(items) * Hs * Ws * 3)
            futs: List[Future] = []
            if decode:
                self._wait(s)
                if self._ring[s] is None or self._ring[s].numel() < used:
                    self._ring[s] = torch.empty(used, dtype=torch.uint8).pin_memory()
                host = self._ring[s].numpy()
                for Hs, Ws, off, keys, paths in layout:
                    n = Hs * Ws * 3
                    for i, (key, path) in enumerate(zip(keys, paths)):
                        dst = host[off + i * n:off + (i + 1) * n].reshape(Hs, Ws, 3)
                        futs.append(self._start(_decode, path, dst))
                        self._inflight[key] = j
            self._pending[j] = {"scan": scan, "ref": ref, "vids": vids, "have": have, "borrow": borrow, "layout": layout, "used": used,
                                "futs": futs}
            self._scheduled += 1

    def __next__(self) -> Dict[str, object]:
        from . import ops
        if self._closed or self._k >= len(self.order):
            self.close()
            raise StopIteration
        k = self._k
        try:
            self._schedule(k + self.ahead + 1)
            rec = self._pending.pop(k)
            for f in rec["futs"]:
                f.result()
            sc, scan = self.scenes, rec["scan"]
            views: Dict[tuple, Tensor] = dict(rec["have"])
            with torch.cuda.device(self.device):
                if rec["layout"]:
                    s = k % (self.ahead + 1)
                    staged = self._ring[s][:rec["used"]].to(self.device, non_blocking=True)     # the one copy, on the current stream
                    self._record(s)
                    for Hs, Ws, off, keys, _ in rec["layout"]:
                        V = len(keys)
                        rows, cols = view_tables(Hs, Ws, self.pad, sc.max_h, sc.max_w, self.device)
                        out = ops.eval_views(staged[off:off + V * Hs * Ws * 3].view(V, Hs, Ws, 3), rows, cols)
                        for i, key in enumerate(keys):
                            t = out[i].clone() if V > 1 else out[0]      # its own memory: an eviction frees what the cache counts
                            views[key] = self._ready[key] = t
                            self.cache.put(key, t, self.view_bytes)
                            del self._inflight[key]
                for key in rec["borrow"]:
                    views[key] = self._ready[key]
                imgs = torch.stack([views[(scan, vid)] for vid in rec["vids"]]).unsqueeze(0)
            wanted = {key for r in self._pending.values() for key in r["borrow"]}
            for key in [key for key in self._ready if key not in wanted]:
                del self._ready[key]
            cams = [self._camera(scan, vid) for vid in rec["vids"]]
            base = np.stack([c[0] for c in cams])
            dmin, dint = cams[0][1], cams[0][2]
            depth_values = np.arange(dmin, dint * (sc.ndepths - 0.5) + dmin, dint, dtype=np.float32)
            self._k += 1
            return {"imgs": imgs, "proj_matrices": self._stages(base), "depth_values": depth_values,
                    "filename": scan + "/{}/" + f"{rec['ref']:08d}" + "{}"}
        except BaseException:
            self.close()
            raise


# ---------------------------------------------------------------------------------------------------------------------
# outputs
def _write_files(outdir: str, filename: str, depth: np.ndarray, conf3: np.ndarray, cam: np.ndarray, img_u8: np.ndarray,
                 stages: Sequence[np.ndarray]) -> None:
    """The files of ``mvs_io.save_outputs`` (and of ``infer --save_stages``) from arrays that are already packed."""
    from PIL import Image
    paths = {k: os.path.join(outdir, filename.format(k, ext)) for k, ext in
             (("depth_est", ".pfm"), ("confidence", ".pfm"), ("cams", "_cam.txt"), ("images", ".jpg"))}
    for p in paths.values():
        os.makedirs(os.path.dirname(p), exist_ok=True)
    mvs_io.write_pfm(paths["depth_est"], depth)
    mvs_io.write_pfm(paths["confidence"], conf3)
    mvs_io.write_cam_file(paths["cams"], cam)
    Image.fromarray(img_u8).save(paths["images"], quality=95)
    for k, d in enumerate(stages, 1):
        p = os.path.join(outdir, filename.format(f"depth_stage{k}", ".pfm"))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        mvs_io.write_pfm(p, d)


class OutputWriter:
    """Writes the outputs of depth maps while the next forward runs.

    ``submit`` (caller's thread, caller's current stream) launches ``ops.eval_outputs``, copies the depth map, ``conf3``, ``img_u8``
    and with ``save_stages`` the three stage depth maps into one of ``depth`` sets of pinned buffers with ``non_blocking`` copies,
    records an event and queues the job; it does not wait for the device.  ONE writer thread waits for the event and writes the files
    (``mvs_io.write_pfm`` / ``write_cam_file``, ``Image.save(quality=95)``), then hands the buffers back.  At most ``depth`` jobs are in
    flight: ``submit`` blocks when all buffer sets are taken.  An error in the writer is kept (every later job is dropped, its buffers
    released, so nothing blocks) and re-raised once, by the next ``submit`` or by ``close()``; ``close()`` returns only when every job is on
    disk and the thread has ended.  ``write`` replaces the function that writes one job's files (tests)."""

    def __init__(self, outdir: str, depth: int = 3, write=None):
        if int(depth) < 1:
            raise ValueError("OutputWriter: depth must be >= 1")
        self.outdir, self.depth = str(outdir), int(depth)
        self._write = write if write is not None else _write_files
        self._free: "queue.Queue[dict]" = queue.Queue()
        for _ in range(self.depth):
            self._free.put({})
        self._jobs: "queue.Queue[Optional[tuple]]" = queue.Queue()
        self._error: Optional[BaseException] = None
        self._failed = False                                  # sticky: after a failure the thread only hands buffers back
        self._closed = False
        self._thread = threading.Thread(target=self._run, name="cds-eval-writer", daemon=True)
        self._thread.start()

    def __enter__(self) -> "OutputWriter":
        return self

    def __exit__(self, *exc) -> bool:
        if exc[0] is None:
            self.close()
        else:                                                 # already failing: do not mask that error with the writer's
            try:
                self.close()
            except Exception:
                pass
        return False

    def _run(self) -> None:
        while True:
            job = self._jobs.get()
            if job is None:
                return
            slot, event, filename, cam, names = job
            try:
                if not self._failed:
                    if event is not None:
                        event.synchronize()
                    arrays = {n: slot[n].numpy() for n in names}
                    self._write(self.outdir, filename, arrays["depth"], arrays["conf3"], cam, arrays["img_u8"],
                                [arrays[n] for n in names if n.startswith("stage")])
            except BaseException as e:                        # kept for the caller's thread
                self._failed, self._error = True, e
            finally:
                self._free.put(slot)

    def _raise(self) -> None:
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    @staticmethod
    def _stage(slot: dict, name: str, src: Tensor) -> None:
        """src (device, or host in a test) -> the slot's pinned buffer of that name, without blocking the host."""
        buf = slot.get(name)
        if buf is None or buf.shape != src.shape or buf.dtype != src.dtype:
            buf = torch.empty(src.shape, dtype=src.dtype)
            buf = slot[name] = buf.pin_memory() if src.is_cuda else buf
        buf.copy_(src, non_blocking=True)

    def submit_packed(self, filename: str, cam: np.ndarray, parts: Sequence[Tuple[str, Tensor]]) -> None:
        """Queue one job from tensors that are already packed: parts = ("depth", [h,w] float32), ("conf3", [h,w,3] float32),
        ("img_u8", [h,w,3] uint8) and optionally ("stage1" .. "stage3", float32 maps), on the device (copied on the current stream of
        their device, which must be the current device) or on the host."""
        if self._closed:
            raise RuntimeError("OutputWriter: submit after close")
        self._raise()
        slot = self._free.get()                               # blocks while `depth` jobs are in flight
        try:
            for name, t in parts:
                self._stage(slot, name, t)
            event = None
            if any(t.is_cuda for _, t in parts):
                event = torch.cuda.Event()
                event.record()
        except BaseException:
            self._free.put(slot)
            raise
        self._jobs.put((slot, event, filename, np.array(cam, copy=True), [n for n, _ in parts]))

    def submit(self, filename: str, out: Dict[str, object], cam: np.ndarray, ref_img: Tensor, save_stages: bool = False) -> None:
        """out: the model's output dict of ONE sample (batch 1); cam [2,4,4]: the reference view's matrices at the depth map's scale;
        ref_img [3,H,W]: the reference view on the device."""
        from . import ops
        depth = out["refined_depth"][0].float()
        confs = [out["stage1"]["photometric_confidence"][0].float().contiguous(),
                 out["stage2"]["photometric_confidence"][0].float().contiguous(),
                 out["photometric_confidence"][0].float().contiguous()]
        ref_img = ref_img.float().contiguous()
        h, w = int(depth.shape[0]), int(depth.shape[1])
        with torch.cuda.device(depth.device):
            tab = output_tables([tuple(c.shape) for c in confs] + [tuple(ref_img.shape[1:])], h, w, depth.device)
            conf3, img_u8 = ops.eval_outputs(confs, ref_img, tab, h, w)
            parts = [("depth", depth), ("conf3", conf3), ("img_u8", img_u8)]
            if save_stages:
                parts += [(f"stage{k}", out[f"stage{k}"]["depth"][0].float()) for k in (1, 2, 3)]
            self.submit_packed(filename, cam, parts)

    def close(self) -> None:
        """Wait until every submitted job is on disk, end the thread, re-raise a writer error.  Idempotent."""
        if not self._closed:
            self._closed = True
            self._jobs.put(None)
            self._thread.join()
        self._raise()
