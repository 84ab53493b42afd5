"""COLMAP sparse model -> MVSNet-format scene: the reference's ``colmap2mvsnet.py`` with the view selection on the GPU.

    python -m cds_mvsnet_amd.colmap --dense_folder <colmap dense dir> --save_folder <scene dir>
           [--max_d 192] [--interval_scale 1] [--theta0 5] [--sigma1 1] [--sigma2 10] [--model_ext .bin|.txt]

reads ``<dense>/images/*`` and ``<dense>/sparse/{cameras,images,points3D}{.bin,.txt}`` (what COLMAP's ``image_undistorter``
writes) and writes ``<save>/cams/%08d_cam.txt``, ``<save>/pair.txt`` and ``<save>/images_post/%08d.jpg``: the layout
``mvs_io.EvalScenes`` reads, so ``python -m cds_mvsnet_amd.infer --dataset general --testpath <parent of save> ...`` runs on it.

The rule (the reference's, colmap2mvsnet.py:295-449, float64 throughout):

1. Images are renumbered 0..N-1 in ascending COLMAP image id.
2. Intrinsic [[fx,0,cx],[0,fy,cy],[0,0,1]] from the camera's first parameters (``f`` stands for fx and fy); distortion
   parameters are ignored.  Extrinsic [R(qvec) | tvec].
3. Depth range of image i: z = row 2 of the extrinsic applied to every observation whose point id is not -1 (duplicates
   count), ascending; num_min = max(1, int(0.03 n)), num_max = max(5, int(0.1 n)); depth_min = mean of the lowest num_min,
   depth_max = mean of the highest num_max values (both slices clip at n, both summed in ascending order).
   depth_num = max_d, or for max_d == 0 the fractional inverse-depth plane count of colmap2mvsnet.py:379-390;
   interval = (depth_max - depth_min) / (depth_num - 1) / interval_scale.
4. Pair score for i < j: S[i,j] = S[j,i] = sum of w(theta_p) over the valid point ids both images observe, each id once per
   occurrence in image i (the lower index); theta_p = the angle in degrees at p between the camera centres c = -R^T t;
   w = exp(-(theta - theta0)^2 / (2 sigma^2)), sigma = sigma1 if theta <= theta0 else sigma2.
5. For every i the 10 entries of row i with the highest score over all k (k = i, score 0, included), descending; equal
   scores higher index first.
6. Cam files: every extrinsic / intrinsic entry as ``str(float64)`` and a space, last line ``'%f %f %f %f'`` of (depth_min,
   interval, depth_num, depth_max).  ``pair.txt`` as the reference prints it, scores as ``%f``.  An image whose name ends
   in ``.jpg`` is copied, any other is re-encoded with PIL.  ``cams/`` and ``images_post/`` of the save folder are replaced.

Where the reference leaves the behaviour open, this module fixes it:

* the cosine is clamped to [-1, 1] before ``acos`` (the reference gets NaN for a cosine that rounds above 1; the NaN
  poisons the pair's score and then sorts first);
* a point that coincides with one of the two camera centres contributes nothing (the reference divides by zero);
* an image without a valid observation raises ``ValueError`` (the reference divides by zero), as does a point id that
  ``points3D`` does not hold (the reference raises ``KeyError``), and a save folder that is the dense folder is refused.

Steps 3 and 4 run in ``csrc/colmap.hip`` (``ops.colmap_depth_ranges``, ``ops.colmap_pair_scores``); there is no CPU path.
The pair scores are accumulated in multi-limb 64-bit fixed point (40-bit limbs, as many as the smallest weight of the given
theta0 and sigmas needs: 7 at the defaults, where w spans 221 binary orders), and the reference ranks images that share a point at any angle above images that share nothing.  Each term enters
with an error below q = 2^-80 (``ops.COLMAP_SCORE_QUANTUM``), and the matrix is bit-identical from run to run.  Reading, the selection of step 5,
the plane count for max_d == 0 and the writers are host code (an N x N matrix and N scalars).
"""
from __future__ import annotations

import argparse
import collections
import os
import shutil
import struct
from typing import Dict, List, Sequence, Tuple

import numpy as np

Camera = collections.namedtuple("Camera", ["id", "model", "width", "height", "params"])
Image = collections.namedtuple("Image", ["id", "qvec", "tvec", "camera_id", "name", "xys", "point3D_ids"])


class Points3D:
    """The points of a model as arrays (a dict of a million small objects is what makes the reference's reader slow):
    ids [P] int64 ascending, xyz [P,3] float64, rgb [P,3] uint8, error [P] float64 and the tracks as a CSR: track_ptr [P+1]
    int64 into track_image_ids / track_point2D_idxs [T] int32."""

    def __init__(self, ids, xyz, rgb, error, track_ptr, track_image_ids, track_point2D_idxs):
        ids = np.asarray(ids, np.int64).reshape(-1)
        P = ids.size
        self.ids = ids
        self.xyz = np.asarray(xyz, np.float64).reshape(P, 3)
        self.rgb = np.asarray(rgb, np.uint8).reshape(P, 3)
        self.error = np.asarray(error, np.float64).reshape(P)
        self.track_ptr = np.asarray(track_ptr, np.int64).reshape(P + 1)
        self.track_image_ids = np.asarray(track_image_ids, np.int32).reshape(-1)
        self.track_point2D_idxs = np.asarray(track_point2D_idxs, np.int32).reshape(-1)
        if self.track_ptr[0] != 0 or self.track_ptr[-1] != self.track_image_ids.size or \
                self.track_image_ids.size != self.track_point2D_idxs.size or (np.diff(self.track_ptr) < 0).any():
            raise ValueError("Points3D: track_ptr does not describe the track arrays")
        if P > 1 and (np.diff(ids) <= 0).any():          # keep the ids ascending: lookups are binary searches
            order = np.argsort(ids, kind="stable")
            if (np.diff(ids[order]) == 0).any():
                raise ValueError("Points3D: duplicate point id")
            lens = np.diff(self.track_ptr)[order]
            starts = self.track_ptr[:-1][order]
            ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            gather = np.repeat(starts - ptr[:-1], lens) + np.arange(ptr[-1])
            self.ids, self.xyz, self.rgb, self.error = ids[order], self.xyz[order], self.rgb[order], self.error[order]
            self.track_ptr = ptr
            self.track_image_ids, self.track_point2D_idxs = self.track_image_ids[gather], self.track_point2D_idxs[gather]

    def __len__(self) -> int:
        return int(self.ids.size)

    def track(self, k: int) -> Tuple[np.ndarray, np.ndarray]:
        s, e = self.track_ptr[k], self.track_ptr[k + 1]
        return self.track_image_ids[s:e], self.track_point2D_idxs[s:e]

    def __eq__(self, other) -> bool:
        return isinstance(other, Points3D) and all(
            np.array_equal(getattr(self, k), getattr(other, k))
            for k in ("ids", "xyz", "rgb", "error", "track_ptr", "track_image_ids", "track_point2D_idxs"))


# model id -> (name, number of parameters); the first parameters are (f | fx fy) cx cy, the rest is distortion
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
CAMERA_MODEL_IDS = {name: (mid, n) for mid, (name, n) in CAMERA_MODELS.items()}
SINGLE_FOCAL = {"SIMPLE_PINHOLE", "SIMPLE_RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL", "RADIAL_FISHEYE"}
NUM_SELECTED = 10
_OBS = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
_P3D_HEAD = np.dtype([("id", "<u8"), ("xyz", "<f8", 3), ("rgb", "u1", 3), ("error", "<f8"), ("len", "<u8")])   # 51 bytes
_TRACK = np.dtype([("image", "<i4"), ("idx", "<i4")])


# ------------------------------------------------------------------------------------------------------------ readers
def _data_lines(path: str):
    with open(path) as f:
        for line in f:
            yield line


def read_cameras_text(path: str) -> Dict[int, Camera]:
    cameras = {}
    for line in _data_lines(path):
        e = line.split()
        if not e or e[0].startswith("#"):
            continue
        if e[1] not in CAMERA_MODEL_IDS:
            raise ValueError(f"{path}: unknown camera model {e[1]}")
        cameras[int(e[0])] = Camera(int(e[0]), e[1], int(e[2]), int(e[3]), np.array([float(v) for v in e[4:]], np.float64))
    return cameras


def read_cameras_binary(path: str) -> Dict[int, Camera]:
    with open(path, "rb") as f:
        buf = f.read()
    (n,), o = struct.unpack_from("<Q", buf, 0), 8
    cameras = {}
    for _ in range(n):
        cid, mid, w, h = struct.unpack_from("<iiQQ", buf, o)
        if mid not in CAMERA_MODELS:
            raise ValueError(f"{path}: unknown camera model id {mid}")
        name, k = CAMERA_MODELS[mid]
        cameras[cid] = Camera(cid, name, w, h, np.frombuffer(buf, "<f8", k, o + 24).astype(np.float64))
        o += 24 + 8 * k
    return cameras


def read_images_text(path: str) -> Dict[int, Image]:
    images = {}
    lines = _data_lines(path)
    for line in lines:
        e = line.split()
        if not e or e[0].startswith("#"):
            continue
        obs = next(lines, "").split()
        xys = np.empty((len(obs) // 3, 2), np.float64)
        xys[:, 0] = np.array(obs[0::3], np.float64) if obs else 0
        xys[:, 1] = np.array(obs[1::3], np.float64) if obs else 0
        ids = np.array([int(v) for v in obs[2::3]], np.int64)
        images[int(e[0])] = Image(int(e[0]), np.array([float(v) for v in e[1:5]]), np.array([float(v) for v in e[5:8]]),
                                  int(e[8]), e[9], xys, ids)
    return images


def read_images_binary(path: str) -> Dict[int, Image]:
    with open(path, "rb") as f:
        buf = f.read()
    (n,), o = struct.unpack_from("<Q", buf, 0), 8
    images = {}
    for _ in range(n):
        v = struct.unpack_from("<i7di", buf, o)
        o += 64
        end = buf.index(b"\x00", o)
        name = buf[o:end].decode("utf-8")
        (m,) = struct.unpack_from("<Q", buf, end + 1)
        o = end + 9
        obs = np.frombuffer(buf, _OBS, m, o)               # all observations of the image at once
        o += 24 * m
        xys = np.stack([obs["x"], obs["y"]], 1).astype(np.float64)
        images[v[0]] = Image(v[0], np.array(v[1:5]), np.array(v[5:8]), v[8], name, xys, obs["id"].astype(np.int64))
    return images


def read_points3D_text(path: str) -> Points3D:
    ids, xyz, rgb, err, lens, tracks = [], [], [], [], [], []
    for line in _data_lines(path):
        e = line.split()
        if not e or e[0].startswith("#"):
            continue
        ids.append(int(e[0]))
        xyz.append([float(v) for v in e[1:4]])
        rgb.append([int(v) for v in e[4:7]])
        err.append(float(e[7]))
        t = [int(v) for v in e[8:]]
        lens.append(len(t) // 2)
        tracks.extend(t)
    tr = np.array(tracks, np.int64).reshape(-1, 2)
    return Points3D(ids, np.array(xyz, np.float64).reshape(-1, 3), np.array(rgb, np.int64).reshape(-1, 3), err,
                    np.concatenate([[0], np.cumsum(lens)]), tr[:, 0], tr[:, 1])


_BLOCK = 1 << 16      # records per gather: the index array of a block stays at a few tens of MB whatever the model's size


def _gather_records(raw: np.ndarray, offs: np.ndarray, size: int) -> np.ndarray:
    """The ``size``-byte records at byte offsets ``offs`` of ``raw`` as one contiguous uint8 array [len(offs) * size]."""
    out = np.empty((len(offs), size), np.uint8)
    span = np.arange(size)
    for b in range(0, len(offs), _BLOCK):
        out[b:b + _BLOCK] = raw[offs[b:b + _BLOCK, None] + span]
    return out.reshape(-1)


def _scatter_records(out: np.ndarray, offs: np.ndarray, records: np.ndarray) -> None:
    """The inverse: ``records`` [n, size] uint8 written at byte offsets ``offs`` of ``out``."""
    span = np.arange(records.shape[1])
    for b in range(0, len(offs), _BLOCK):
        out[offs[b:b + _BLOCK, None] + span] = records[b:b + _BLOCK]


def read_points3D_binary(path: str) -> Points3D:
    with open(path, "rb") as f:
        buf = f.read()
    (P,) = struct.unpack_from("<Q", buf, 0)
    # the records have variable length, so their offsets are found one after another (one integer per point); everything
    # else is gathered in bulk
    offs = np.empty(P, np.int64)
    o, unpack = 8, struct.Struct("<Q").unpack_from
    for k in range(P):
        offs[k] = o
        o += 51 + 8 * unpack(buf, o + 43)[0]
    if o != len(buf):
        raise ValueError(f"{path}: {len(buf)} bytes, the records end at {o}")
    raw = np.frombuffer(buf, np.uint8)
    head = _gather_records(raw, offs, 51).view(_P3D_HEAD).reshape(P)
    lens = head["len"].astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    first = np.repeat(offs + 51 - 8 * ptr[:-1], lens) + 8 * np.arange(ptr[-1])       # byte offset of every track element
    tr = _gather_records(raw, first, 8).view(_TRACK).reshape(-1)
    return Points3D(head["id"].astype(np.int64), head["xyz"], head["rgb"], head["error"], ptr, tr["image"], tr["idx"])


def read_model(path: str, ext: str = ".bin") -> Tuple[Dict[int, Camera], Dict[int, Image], Points3D]:
    """``<path>/{cameras,images,points3D}<ext>`` -> (cameras {id: Camera}, images {id: Image}, Points3D)."""
    if ext not in (".txt", ".bin"):
        raise ValueError(f"model extension {ext!r}: .txt or .bin")
    rc, ri, rp = (read_cameras_text, read_images_text, read_points3D_text) if ext == ".txt" else \
        (read_cameras_binary, read_images_binary, read_points3D_binary)
    return rc(os.path.join(path, "cameras" + ext)), ri(os.path.join(path, "images" + ext)), \
        rp(os.path.join(path, "points3D" + ext))


# ------------------------------------------------------------------------------------------------------------ writers
def _r(v) -> str:
    return repr(float(v))                 # shortest text that reads back to the same float64


def model_bytes(ext: str, cameras: Dict[int, Camera], images: Dict[int, Image], points3D: Points3D) -> Dict[str, bytes]:
    """The three files of a model as {"cameras<ext>": bytes, ...}; floats in the text form are written with ``repr`` so that
    both formats hold the same model."""
    if ext == ".txt":
        cam = ["# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n"
               f"# Number of cameras: {len(cameras)}\n"]
        for c in cameras.values():
            cam.append(" ".join([str(c.id), c.model, str(int(c.width)), str(int(c.height))] + [_r(v) for v in c.params]) + "\n")
        img = ["# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
               f"#   POINTS2D[] as (X, Y, POINT3D_ID)\n# Number of images: {len(images)}\n"]
        for im in images.values():
            img.append(" ".join([str(im.id)] + [_r(v) for v in im.qvec] + [_r(v) for v in im.tvec] +
                                [str(im.camera_id), im.name]) + "\n")
            img.append(" ".join(f"{_r(x)} {_r(y)} {int(p)}" for (x, y), p in zip(im.xys, im.point3D_ids)) + "\n")
        pts = ["# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, "
               f"TRACK[] as (IMAGE_ID, POINT2D_IDX)\n# Number of points: {len(points3D)}\n"]
        for k in range(len(points3D)):
            ti, tp = points3D.track(k)
            pts.append(" ".join([str(int(points3D.ids[k]))] + [_r(v) for v in points3D.xyz[k]] +
                                [str(int(v)) for v in points3D.rgb[k]] + [_r(points3D.error[k])] +
                                [f"{int(a)} {int(b)}" for a, b in zip(ti, tp)]) + "\n")
        return {"cameras.txt": "".join(cam).encode(), "images.txt": "".join(img).encode(),
                "points3D.txt": "".join(pts).encode()}
    if ext != ".bin":
        raise ValueError(f"model extension {ext!r}: .txt or .bin")
    cam = [struct.pack("<Q", len(cameras))]
    for c in cameras.values():
        mid, k = CAMERA_MODEL_IDS[c.model]
        if len(c.params) != k:
            raise ValueError(f"camera {c.id}: {c.model} has {k} parameters, got {len(c.params)}")
        cam.append(struct.pack("<iiQQ", c.id, mid, int(c.width), int(c.height)) + np.asarray(c.params, "<f8").tobytes())
    img = [struct.pack("<Q", len(images))]
    for im in images.values():
        obs = np.empty(len(im.point3D_ids), _OBS)
        obs["x"], obs["y"], obs["id"] = im.xys[:, 0], im.xys[:, 1], im.point3D_ids
        img.append(struct.pack("<i7di", im.id, *[float(v) for v in im.qvec], *[float(v) for v in im.tvec], im.camera_id) +
                   im.name.encode("utf-8") + b"\x00" + struct.pack("<Q", obs.size) + obs.tobytes())
    P = len(points3D)
    head = np.zeros(P, _P3D_HEAD)
    head["id"], head["xyz"], head["rgb"], head["error"] = points3D.ids, points3D.xyz, points3D.rgb, points3D.error
    lens = np.diff(points3D.track_ptr)
    head["len"] = lens
    tr = np.empty(points3D.track_image_ids.size, _TRACK)
    tr["image"], tr["idx"] = points3D.track_image_ids, points3D.track_point2D_idxs
    out = np.empty(51 * P + 8 * tr.size, np.uint8)        # records interleaved: 51-byte head, then the track
    offs = 51 * np.arange(P) + 8 * points3D.track_ptr[:-1]
    _scatter_records(out, offs, head.view(np.uint8).reshape(P, 51))
    first = np.repeat(offs + 51 - 8 * points3D.track_ptr[:-1], lens) + 8 * np.arange(tr.size)
    _scatter_records(out, first, tr.view(np.uint8).reshape(-1, 8))
    return {"cameras.bin": b"".join(cam), "images.bin": b"".join(img),
            "points3D.bin": struct.pack("<Q", P) + out.tobytes()}


def write_model(path: str, ext: str, cameras: Dict[int, Camera], images: Dict[int, Image], points3D: Points3D) -> None:
    """Write ``<path>/{cameras,images,points3D}<ext>`` (``.txt`` or ``.bin``) so that :func:`read_model` returns the same model."""
    os.makedirs(path, exist_ok=True)
    for name, data in model_bytes(ext, cameras, images, points3D).items():
        with open(os.path.join(path, name), "wb") as f:
            f.write(data)


# ----------------------------------------------------------------------------------------------------- cameras (host)
def image_order(images: Dict[int, Image]) -> List[int]:
    """COLMAP image ids in ascending order: position = the scene's image number (step 1)."""
    return sorted(images.keys())


def intrinsic_matrix(cam: Camera) -> np.ndarray:
    if cam.model not in CAMERA_MODEL_IDS:
        raise ValueError(f"camera {cam.id}: unknown model {cam.model}")
    p = np.asarray(cam.params, np.float64)
    fx, fy, cx, cy = (p[0], p[0], p[1], p[2]) if cam.model in SINGLE_FOCAL else (p[0], p[1], p[2], p[3])
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)


def rotation_matrix(q: np.ndarray) -> np.ndarray:
    """Rotation of a COLMAP quaternion (w, x, y, z), evaluated as the reference evaluates it."""
    w, x, y, z = (np.float64(v) for v in q)
    return np.array([[1 - 2 * y ** 2 - 2 * z ** 2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x ** 2 - 2 * z ** 2, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x ** 2 - 2 * y ** 2]], np.float64)


def scene_cameras(cameras: Dict[int, Camera], images: Dict[int, Image]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (extrinsics [N,4,4], intrinsics [N,3,3], centres [N,3] = -R^T t), float64, in scene order (step 2)."""
    order = image_order(images)
    ext = np.zeros((len(order), 4, 4))
    intr = np.zeros((len(order), 3, 3))
    for i, iid in enumerate(order):
        im = images[iid]
        if im.camera_id not in cameras:
            raise ValueError(f"image {iid} ({im.name}): camera {im.camera_id} is not in the model")
        ext[i, :3, :3] = rotation_matrix(im.qvec)
        ext[i, :3, 3] = im.tvec
        ext[i, 3, 3] = 1
        intr[i] = intrinsic_matrix(cameras[im.camera_id])
    centres = -np.einsum("nji,nj->ni", ext[:, :3, :3], ext[:, :3, 3])
    if not (np.isfinite(ext).all() and np.isfinite(intr).all()):
        raise ValueError("the model holds a camera or a pose that is not finite")
    return ext, intr, centres


def flatten_observations(images: Dict[int, Image], points3D: Points3D) -> Tuple[np.ndarray, np.ndarray]:
    """The valid observations (point id != -1) of all images in scene order: (obs_img [E] int32 image number, obs_pt [E]
    int64 index into ``points3D.ids``), duplicates kept.  ValueError for an image without one and for a dangling point id."""
    imgs, pts = [], []
    for i, iid in enumerate(image_order(images)):
        im = images[iid]
        pid = np.asarray(im.point3D_ids, np.int64)
        pid = pid[pid != -1]
        if pid.size == 0:
            raise ValueError(f"image {iid} ({im.name}) has no observation of a 3D point: it has no depth range")
        k = np.searchsorted(points3D.ids, pid)
        bad = (k >= len(points3D)) | (points3D.ids[np.minimum(k, len(points3D) - 1)] != pid) if len(points3D) else \
            np.ones(pid.size, bool)
        if bad.any():
            raise ValueError(f"image {iid} ({im.name}) observes point {int(pid[bad][0])}, which points3D does not hold")
        imgs.append(np.full(pid.size, i, np.int32))
        pts.append(k.astype(np.int64))
    if not imgs:
        raise ValueError("the model has no images")
    return np.concatenate(imgs), np.concatenate(pts)


def range_counts(n: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(num_min, num_max) of step 3 for per-image observation counts n: max(1, int(0.03 n)), max(5, int(0.1 n))."""
    n = np.asarray(n, np.float64)
    return np.maximum(1, (n * 0.03).astype(np.int64)).astype(np.int32), np.maximum(5, (n * 0.1).astype(np.int64)).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------- GPU steps
def _device_observations(images, points3D, device):
    import torch
    obs_img, obs_pt = flatten_observations(images, points3D)
    if not np.isfinite(points3D.xyz).all():
        raise ValueError("points3D holds a coordinate that is not finite")
    return (torch.from_numpy(obs_img).to(device), torch.from_numpy(obs_pt).to(device),
            torch.from_numpy(np.ascontiguousarray(points3D.xyz)).to(device), np.bincount(obs_img))


def depth_ranges(cameras, images, points3D, device: str = "cuda", _obs=None) -> np.ndarray:
    """(depth_min, depth_max) [N,2] float64 of step 3, on the GPU."""
    import torch
    from . import ops
    ext = scene_cameras(cameras, images)[0]
    obs_img, obs_pt, xyz, counts = _obs or _device_observations(images, points3D, device)
    nmin, nmax = range_counts(counts)
    with torch.cuda.device(xyz.device):
        out = ops.colmap_depth_ranges(obs_img, obs_pt, xyz, torch.from_numpy(np.ascontiguousarray(ext[:, 2, :])).to(xyz.device),
                                      torch.from_numpy(nmin).to(xyz.device), torch.from_numpy(nmax).to(xyz.device))
    return out.cpu().numpy()


def pair_scores(cameras, images, points3D, theta0: float = 5.0, sigma1: float = 1.0, sigma2: float = 10.0,
                device: str = "cuda", _obs=None):
    """The score matrix of step 4 on the GPU -> torch float64 [N,N] on the device (symmetric, zero diagonal)."""
    import torch
    from . import ops
    centres = scene_cameras(cameras, images)[2]
    obs_img, obs_pt, xyz, _ = _obs or _device_observations(images, points3D, device)
    with torch.cuda.device(xyz.device):
        return ops.colmap_pair_scores(obs_img, obs_pt, xyz, torch.from_numpy(centres).to(xyz.device), theta0, sigma1, sigma2)[0]


# ------------------------------------------------------------------------------------------- host: selection and files
def plane_count(intrinsic: np.ndarray, extrinsic: np.ndarray, depth_min: float, depth_max: float) -> float:
    """The reference's inverse-depth plane count for max_d == 0 (fractional): the planes between depth_min and depth_max
    whose spacing is one pixel of disparity at the principal point."""
    R, t = extrinsic[:3, :3], extrinsic[:3, 3]
    p1 = [intrinsic[0, 2], intrinsic[1, 2], 1]
    p2 = [intrinsic[0, 2] + 1, intrinsic[1, 2], 1]
    P1 = np.matmul(np.linalg.inv(R), np.matmul(np.linalg.inv(intrinsic), p1) * depth_min - t)
    P2 = np.matmul(np.linalg.inv(R), np.matmul(np.linalg.inv(intrinsic), p2) * depth_min - t)
    return (1 / depth_min - 1 / depth_max) / (1 / depth_min - 1 / (depth_min + np.linalg.norm(P2 - P1)))


def finish_depth_ranges(min_max: np.ndarray, extrinsics: np.ndarray, intrinsics: np.ndarray, max_d: int = 192,
                        interval_scale: float = 1.0) -> np.ndarray:
    """[N,2] (depth_min, depth_max) -> [N,4] (depth_min, interval, depth_num, depth_max), the last line of the cam files."""
    out = np.zeros((len(min_max), 4))
    for i, (dmin, dmax) in enumerate(np.asarray(min_max, np.float64)):
        num = plane_count(intrinsics[i], extrinsics[i], dmin, dmax) if max_d == 0 else max_d
        out[i] = (dmin, (dmax - dmin) / (num - 1) / interval_scale, num, dmax)
    return out


def select_views(score: np.ndarray, num: int = NUM_SELECTED) -> List[List[Tuple[int, float]]]:
    """Step 5: per row the ``num`` best (index, score), descending, ties higher index first (a stable ascending sort, reversed)."""
    score = np.asarray(score, np.float64)
    return [[(int(k), float(row[k])) for k in np.argsort(row, kind="stable")[::-1][:num]] for row in score]


def write_cam_file(path: str, extrinsic: np.ndarray, intrinsic: np.ndarray, depth_range: Sequence[float]) -> None:
    with open(path, "w") as f:
        f.write("extrinsic\n")
        for row in np.asarray(extrinsic, np.float64):
            f.write("".join(str(v) + " " for v in row) + "\n")
        f.write("\nintrinsic\n")
        for row in np.asarray(intrinsic, np.float64):
            f.write("".join(str(v) + " " for v in row) + "\n")
        f.write("\n%f %f %f %f\n" % tuple(depth_range))


def write_pair_file(path: str, view_sel: List[List[Tuple[int, float]]]) -> None:
    with open(path, "w") as f:
        f.write("%d\n" % len(view_sel))
        for i, sel in enumerate(view_sel):
            f.write("%d\n%d " % (i, len(sel)))
            for k, s in sel:
                f.write("%d %f " % (k, s))
            f.write("\n")


def write_scene(save_folder: str, extrinsics: np.ndarray, intrinsics: np.ndarray, ranges: np.ndarray,
                score: np.ndarray) -> None:
    """``cams/%08d_cam.txt`` (the folder is replaced) and ``pair.txt`` from per-image cameras, [N,4] depth ranges and the
    [N,N] score matrix."""
    cam_dir = os.path.join(save_folder, "cams")
    if os.path.exists(cam_dir):
        shutil.rmtree(cam_dir)
    os.makedirs(cam_dir)
    for i in range(len(extrinsics)):
        write_cam_file(os.path.join(cam_dir, "%08d_cam.txt" % i), extrinsics[i], intrinsics[i], ranges[i])
    write_pair_file(os.path.join(save_folder, "pair.txt"), select_views(score))


def convert_images(image_dir: str, save_folder: str, images: Dict[int, Image]) -> None:
    """``images_post/%08d.jpg`` (the folder is replaced): a copy of every image named ``*.jpg``, a PIL re-encoding of any other."""
    out_dir = os.path.join(save_folder, "images_post")
    if os.path.exists(out_dir):
        shutil.rmtree(out_dir)
    os.makedirs(out_dir)
    for i, iid in enumerate(image_order(images)):
        src, dst = os.path.join(image_dir, images[iid].name), os.path.join(out_dir, "%08d.jpg" % i)
        if src.endswith(".jpg"):
            shutil.copyfile(src, dst)
        else:
            from PIL import Image as PILImage
            PILImage.open(src).convert("RGB").save(dst, quality=95)


def _same_folder(a: str, b: str) -> bool:
    return os.path.realpath(a) == os.path.realpath(b)


def convert(dense_folder: str, save_folder: str, max_d: int = 192, interval_scale: float = 1.0, theta0: float = 5.0,
            sigma1: float = 1.0, sigma2: float = 10.0, model_ext: str = ".bin", device: str = "cuda") -> Dict[str, object]:
    """The whole conversion.  -> {"images": N, "points": P, "score": [N,N] float64, "ranges": [N,4]} (numpy)."""
    if _same_folder(dense_folder, save_folder):
        raise ValueError(f"--save_folder {save_folder} is the dense folder: the converted images/ would land beside COLMAP's")
    cameras, images, points3D = read_model(os.path.join(dense_folder, "sparse"), model_ext)
    ext, intr, _ = scene_cameras(cameras, images)
    obs = _device_observations(images, points3D, device)
    min_max = depth_ranges(cameras, images, points3D, device, _obs=obs)
    score = pair_scores(cameras, images, points3D, theta0, sigma1, sigma2, device, _obs=obs).cpu().numpy()
    ranges = finish_depth_ranges(min_max, ext, intr, max_d, interval_scale)
    os.makedirs(save_folder, exist_ok=True)
    convert_images(os.path.join(dense_folder, "images"), save_folder, images)
    write_scene(save_folder, ext, intr, ranges, score)
    return {"images": len(images), "points": len(points3D), "score": score, "ranges": ranges}


# ---------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Convert a COLMAP sparse model to an MVSNet-format scene")
    ap.add_argument("--dense_folder", required=True, type=str, help="COLMAP dense folder: images/ and sparse/")
    ap.add_argument("--save_folder", required=True, type=str, help="scene folder to write: cams/, images_post/, pair.txt")
    ap.add_argument("--max_d", type=int, default=192, help="depth planes; 0 = from the inverse-depth rule")
    ap.add_argument("--interval_scale", type=float, default=1)
    ap.add_argument("--theta0", type=float, default=5)
    ap.add_argument("--sigma1", type=float, default=1)
    ap.add_argument("--sigma2", type=float, default=10)
    ap.add_argument("--model_ext", type=str, default=".bin", choices=[".txt", ".bin"], help="sparse model format")
    return ap.parse_args(argv)


def main(argv=None) -> Dict[str, object]:
    a = parse_args(argv)
    out = convert(a.dense_folder, a.save_folder, a.max_d, a.interval_scale, a.theta0, a.sigma1, a.sigma2, a.model_ext)
    print(f"{a.save_folder}: {out['images']} images, {out['points']} sparse points", flush=True)
    return out


if __name__ == "__main__":
    main()
