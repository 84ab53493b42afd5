"""DTU point-cloud evaluation (accuracy / completeness / overall in mm) on the GPU.

Restates the MATLAB evaluation the reference ships (``evaluations/dtu``: BaseEvalMain_web.m, PointCompareMain.m,
reducePts_haa.m, MaxDistCP.m, ComputeStat_web.m) for the fused clouds that ``infer --fuse`` writes:

1. thin the prediction to a minimum spacing ``dst`` = 0.2 mm in a seeded random order (reducePts_haa.m, PointCompareMain.m:7;
   :func:`cds_mvsnet_amd.pointcloud.reduce_points`; MATLAB's ``randperm`` cannot be reproduced, so scores can differ from a
   MATLAB run in the last digits);
2. keep the thinned points whose ObsMask voxel is set (PointCompareMain.m:30-41) and the STL points above the ground plane
   (PointCompareMain.m:51-53), in float64;
3. capped nearest-neighbour distances data -> STL (accuracy) and STL -> data (completeness) (MaxDistCP.m,
   PointCompareMain.m:20-26; :func:`cds_mvsnet_amd.pointcloud.nearest_distance`);
4. mean / median / variance / count of the distances below ``max_dist`` = 20 mm (BaseEvalMain_web.m:63-72,
   ComputeStat_web.m:52-81), overall = (acc + comp) / 2, and over a scan list the mean of the per-scan means.

``python -m cds_mvsnet_amd.dtu_eval --datapath <MVS Data> --plydir <outdir> --scans 1,4,9`` scores a directory of fused
clouds.  The inputs must be float32 ROCm tensors; there is no CPU path.

``--sample_faces [SPACING]`` scores a mesh by its surface: the file is read with ``mesh.read_mesh_ply`` and the samples of its
faces (``mesh.sample_mesh``; SPACING defaults to ``--dst``, a covering radius of 2/3 dst) take the place of its
vertices, which are not added.  Without it a mesh file is scored as the cloud of its vertices, as before.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import struct
import sys
import time
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .mvs_io import read_testlist
from .pointcloud import PointGrid, default_cell, nearest_distance, read_ply_points, reduce_points, thinning_order

Tensor = torch.Tensor

# ---------------------------------------------------------------------------------------------------------------------
# MATLAB v5 MAT-files (what ObsMask<N>_10.mat and Plane<N>.mat hold)
_MI = {1: "i1", 2: "u1", 3: "i2", 4: "u2", 5: "i4", 6: "u4", 7: "f4", 9: "f8", 12: "i8", 13: "u8", 16: "u1"}
_MI_MATRIX, _MI_COMPRESSED = 14, 15
_MX = {6: np.float64, 7: np.float32, 8: np.int8, 9: np.uint8, 10: np.int16, 11: np.uint16, 12: np.int32, 13: np.uint32,
       14: np.int64, 15: np.uint64}
_MX_CHAR = 4
_MX_NAMES = {1: "cell", 2: "struct", 3: "object", 5: "sparse", 16: "function handle", 17: "opaque"}


def load_mat(path: str) -> Dict[str, np.ndarray]:
    """Variables of a MATLAB v5 (``-v6`` / ``-v7``) MAT-file -> {name: numpy array}.  Numeric classes come back in their class
    dtype whatever narrower type the file stores them in (MATLAB writes integral doubles as uint8), logical arrays as bool,
    char arrays as str, N-d arrays reshaped column-major.  Handles zlib-compressed elements, the small-element format,
    8-byte padding and both byte orders.  v7.3 (HDF5) files, v4 files and cell / struct / sparse / object variables raise."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 128:
        raise ValueError(f"{path}: too short for a MAT-file")
    text = data[:116]
    if data[126:128] == b"IM":
        end = "<"
    elif data[126:128] == b"MI":
        end = ">"
    else:
        raise ValueError(f"{path}: not a MATLAB v5 MAT-file (v4 files are not supported)")
    version = struct.unpack(end + "H", data[124:126])[0]
    if version == 0x0200 or b"7.3" in text or data[512:520] == b"\x89HDF\r\n\x1a\n":
        raise ValueError(f"{path}: MATLAB v7.3 (HDF5) MAT-files are not supported; save the variables with -v7")
    if not text.startswith(b"MATLAB"):
        raise ValueError(f"{path}: not a MATLAB v5 MAT-file")
    out: Dict[str, np.ndarray] = {}
    pos = 128
    while pos + 8 <= len(data):
        mtype, body, pos = _element(data, pos, end, path, top=True)
        if mtype == _MI_COMPRESSED:
            inner = zlib.decompress(body)
            mtype, body, _ = _element(inner, 0, end, path)
        if mtype != _MI_MATRIX:
            raise ValueError(f"{path}: unexpected top-level element type {mtype}")
        name, value = _matrix(body, end, path)
        out[name] = value
    return out


def _element(buf: bytes, pos: int, end: str, path: str, top: bool = False) -> Tuple[int, bytes, int]:
    """(type, payload, next position) of the data element at pos."""
    w0, w1 = struct.unpack(end + "II", buf[pos:pos + 8])
    small = w0 >> 16
    if small:                                            # small format: 2-byte size, 2-byte type, 4 bytes of data
        return w0 & 0xFFFF, buf[pos + 4:pos + 4 + small], pos + 8
    mtype, n = w0, w1
    if pos + 8 + n > len(buf):
        raise ValueError(f"{path}: truncated element")
    nxt = pos + 8 + n
    if not (top and mtype == _MI_COMPRESSED):            # compressed elements are not padded
        nxt += (-n) % 8
    return mtype, buf[pos + 8:pos + 8 + n], nxt


def _numeric(buf: bytes, mtype: int, end: str, path: str) -> np.ndarray:
    if mtype not in _MI:
        raise ValueError(f"{path}: unsupported data type {mtype}")
    return np.frombuffer(buf, dtype=np.dtype(_MI[mtype]).newbyteorder(end))


def _matrix(body: bytes, end: str, path: str) -> Tuple[str, object]:
    pos = 0
    t, flags_b, pos = _element(body, pos, end, path)
    flags = _numeric(flags_b, t, end, path)
    cls, logical, cplx = int(flags[0]) & 0xFF, bool(int(flags[0]) & 0x0200), bool(int(flags[0]) & 0x0800)
    t, dims_b, pos = _element(body, pos, end, path)
    dims = tuple(int(d) for d in _numeric(dims_b, t, end, path))
    t, name_b, pos = _element(body, pos, end, path)
    name = bytes(name_b).decode("ascii")
    if cls in _MX_NAMES or (cls not in _MX and cls != _MX_CHAR):
        raise ValueError(f"{path}: variable {name!r} is a {_MX_NAMES.get(cls, f'class {cls}')} array; only numeric, "
                         "logical and char arrays are supported")
    t, real_b, pos = _element(body, pos, end, path)
    real = _numeric(real_b, t, end, path)
    n = int(np.prod(dims)) if dims else 0
    if real.size != n:
        raise ValueError(f"{path}: variable {name!r} holds {real.size} values for dimensions {dims}")
    if cls == _MX_CHAR:
        return name, "".join(chr(c) for c in np.reshape(real, dims, order="F").T.reshape(-1))
    val = np.reshape(real.astype(_MX[cls]), dims, order="F")
    if cplx:
        t, imag_b, pos = _element(body, pos, end, path)
        val = val + 1j * np.reshape(_numeric(imag_b, t, end, path).astype(_MX[cls]), dims, order="F")
    if logical:
        val = val != 0
    return name, val


def load_dtu_scan(datapath: str, n: int) -> Dict[str, np.ndarray]:
    """Ground truth of DTU scan ``n`` under the ``MVS Data`` folder (PointCompareMain.m:10-18,51):
    ``Points/stl/stl%03d_total.ply`` -> ``stl`` float32 [N,3]; ``ObsMask/ObsMask%d_10.mat`` -> ``ObsMask`` bool [X,Y,Z],
    ``BB`` float64 [2,3], ``Res`` float; ``ObsMask/Plane%d.mat`` -> ``P`` float64 [4]."""
    paths = dtu_scan_paths(datapath, n)
    for p in paths.values():
        if not os.path.isfile(p):
            raise FileNotFoundError(f"DTU scan {n}: {p} not found")
    mask = load_mat(paths["obsmask"])
    plane = load_mat(paths["plane"])
    for k, src in (("ObsMask", mask), ("BB", mask), ("Res", mask), ("P", plane)):
        if k not in src:
            raise ValueError(f"DTU scan {n}: variable {k} missing from {paths['plane' if k == 'P' else 'obsmask']}")
    return {"stl": read_ply_points(paths["stl"]), "ObsMask": np.asarray(mask["ObsMask"]).astype(bool),
            "BB": np.asarray(mask["BB"], np.float64).reshape(2, 3), "Res": float(np.asarray(mask["Res"]).reshape(-1)[0]),
            "P": np.asarray(plane["P"], np.float64).reshape(-1)}


def dtu_scan_paths(datapath: str, n: int) -> Dict[str, str]:
    return {"stl": os.path.join(datapath, "Points", "stl", f"stl{n:03d}_total.ply"),
            "obsmask": os.path.join(datapath, "ObsMask", f"ObsMask{n}_10.mat"),
            "plane": os.path.join(datapath, "ObsMask", f"Plane{n}.mat")}


# ---------------------------------------------------------------------------------------------------------------------
def matlab_round(x: Tensor) -> Tensor:
    """MATLAB ``round``: half away from zero (torch.round rounds half to even)."""
    t = torch.trunc(x)                                  # x - trunc(x) is exact; floor(|x| + 0.5) is not (0.5 - 2^-54)
    return t + torch.sign(x) * (torch.abs(x - t) >= 0.5).to(x.dtype)


def data_in_mask(points: Tensor, obs_mask: Tensor, bb: Tensor, res: float) -> Tensor:
    """PointCompareMain.m:30-41 in float64: the voxel ``round((q - BB(1,:)) / Res + 1)`` (1-based) lies inside ObsMask and is
    set.  points [N,3] (any float dtype, device), obs_mask bool [X,Y,Z] (device), bb [2,3] float64 -> bool [N]."""
    qv = matlab_round((points.double() - bb[0].double()) / float(res) + 1.0)
    size = torch.tensor(obs_mask.shape, dtype=torch.float64, device=points.device)
    inside = ((qv > 0) & (qv <= size)).all(1)
    idx = torch.where(inside[:, None], qv - 1.0, torch.zeros_like(qv)).long()
    # sub2ind's column-major index addresses element (i, j, k); obs_mask is indexed as the [X,Y,Z] array it is
    lin = (idx[:, 0] * obs_mask.shape[1] + idx[:, 1]) * obs_mask.shape[2] + idx[:, 2]
    return inside & obs_mask.contiguous().reshape(-1)[lin]


def above_plane(points: Tensor, plane: Tensor) -> Tensor:
    """PointCompareMain.m:53 in float64: ``P' * [q; 1] > 0``.  points [N,3], plane [4] -> bool [N]."""
    p = plane.double().reshape(4)
    q = points.double()
    return (p[0] * q[:, 0] + p[1] * q[:, 1] + p[2] * q[:, 2] + p[3]) > 0


def in_block_grid(points: Tensor, bb: Tensor, block: float) -> Tensor:
    """MaxDistCP.m:5-18 in float64: the point lies in one of the blocks of side ``block`` that tile
    [BB(1,:), BB(1,:) + (floor((BB(2,:) - BB(1,:)) / block) + 1) block).  MaxDistCP gives every other point the distance
    ``block``, so it never counts; that includes masked points up to half a voxel below BB(1,:), which ObsMask's rounding
    still admits.  points [N,3], bb [2,3] -> bool [N]."""
    lo = bb[0].double()
    hi = lo + (torch.floor((bb[1].double() - lo) / block) + 1.0) * block
    q = points.double()
    return ((q >= lo) & (q < hi)).all(1)


def distance_stats(d: Tensor, max_dist: float) -> Dict[str, float]:
    """ComputeStat_web.m:52-68 for one set of distances: keep d < max_dist, then mean, median (mean of the two middle values),
    variance (normalised by n - 1) and count, accumulated in float64.  An empty set gives NaN (variance of one value: 0
    as MATLAB's var)."""
    d = d.double()
    d = d[d < max_dist]
    n = int(d.numel())
    if n == 0:
        return {"mean": math.nan, "median": math.nan, "var": math.nan, "n": 0}
    s = torch.sort(d)[0]
    med = (s[(n - 1) // 2] + s[n // 2]) / 2.0
    mean = d.sum() / n
    var = ((d - mean) ** 2).sum() / (n - 1) if n > 1 else torch.zeros((), dtype=torch.float64)
    return {"mean": float(mean), "median": float(med), "var": float(var), "n": n}


def evaluate(pred_points: Tensor, gt: Dict[str, np.ndarray], dst: float = 0.2, max_dist: float = 20.0, seed: int = 0,
             return_arrays: bool = False, timings: Optional[Dict[str, float]] = None,
             block: Optional[float] = None) -> Dict[str, object]:
    """Score one predicted cloud pred_points [N,3] (float32, device) against ``gt`` from :func:`load_dtu_scan` (keys stl,
    ObsMask, BB, Res, P).  -> {"acc", "comp", "overall", "acc_median", "acc_var", "acc_n", "comp_median", "comp_var",
    "comp_n", "n_points", "n_thinned", "n_in_mask", "n_stl", "n_above_plane"} (+ the per-point arrays with
    ``return_arrays``).  Only the masked data points and the above-plane STL points are queried, with the search capped
    at ``max_dist``; points outside MaxDistCP's block grid (:func:`in_block_grid`, ``block`` = 3 max_dist by default: the
    protocol's 60 mm at max_dist 20, PointCompareMain.m:20) get max_dist as they get 60 there.  ``timings``: a dict that
    receives the device time of each phase in ms (events on the current stream)."""
    if not isinstance(pred_points, torch.Tensor) or not pred_points.is_cuda:
        raise RuntimeError("evaluate: pred_points must be a ROCm (cuda) tensor; there is no CPU fallback")
    dev = pred_points.device
    ev = _Phases(timings)
    stl = torch.as_tensor(np.ascontiguousarray(gt["stl"], dtype=np.float32)).to(dev)
    obs = torch.as_tensor(np.ascontiguousarray(gt["ObsMask"], dtype=bool)).to(dev)
    bb = torch.as_tensor(np.asarray(gt["BB"], np.float64).reshape(2, 3)).to(dev)
    plane = torch.as_tensor(np.asarray(gt["P"], np.float64).reshape(-1)).to(dev)
    pred = pred_points.contiguous()

    ev.mark("upload")
    order = thinning_order(pred.shape[0], seed).to(dev)   # generated on the host (CPU generator)
    ev.mark("order")
    keep = reduce_points(pred, dst, order=order)
    data = pred[keep].contiguous()
    ev.mark("thinning")
    blk = 3.0 * max_dist if block is None else float(block)
    in_mask = data_in_mask(data, obs, bb, float(gt["Res"]))
    above = above_plane(stl, plane)
    q_data = data[in_mask].contiguous()
    q_stl = stl[above].contiguous()
    g_data, g_stl = in_block_grid(q_data, bb, blk), in_block_grid(q_stl, bb, blk)
    ev.mark("masks")
    stl_grid = PointGrid(stl, default_cell(stl)) if stl.shape[0] else None
    data_grid = PointGrid(data, default_cell(data)) if data.shape[0] else None
    ev.mark("grid build")
    ddata = torch.full((q_data.shape[0],), float(max_dist), dtype=torch.float32, device=dev)
    ddata[g_data] = nearest_distance(q_data[g_data].contiguous(), stl, max_dist, grid=stl_grid)
    ev.mark("data->stl")
    dstl = torch.full((q_stl.shape[0],), float(max_dist), dtype=torch.float32, device=dev)
    dstl[g_stl] = nearest_distance(q_stl[g_stl].contiguous(), data, max_dist, grid=data_grid)
    ev.mark("stl->data")
    acc, comp = distance_stats(ddata, max_dist), distance_stats(dstl, max_dist)
    ev.mark("statistics")
    ev.finish()
    res: Dict[str, object] = {
        "acc": acc["mean"], "comp": comp["mean"], "overall": (acc["mean"] + comp["mean"]) / 2.0,
        "acc_median": acc["median"], "acc_var": acc["var"], "acc_n": acc["n"],
        "comp_median": comp["median"], "comp_var": comp["var"], "comp_n": comp["n"],
        "n_points": int(pred.shape[0]), "n_thinned": int(data.shape[0]), "n_in_mask": int(q_data.shape[0]),
        "n_stl": int(stl.shape[0]), "n_above_plane": int(q_stl.shape[0])}
    if return_arrays:
        res.update({"keep": keep, "data": data, "data_in_mask": in_mask, "ddata": ddata, "stl_above_plane": above,
                    "dstl": dstl})
    return res


class _Phases:
    """Device-event timing of the phases of :func:`evaluate` (only when a dict is passed)."""

    def __init__(self, out: Optional[Dict[str, float]]):
        self.out = out
        self.events: List[Tuple[str, torch.cuda.Event]] = []
        if out is not None:
            self._record("start")

    def _record(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.events.append((name, e))

    def mark(self, name):
        if self.out is not None:
            self._record(name)

    def finish(self):
        if self.out is None:
            return
        self.events[-1][1].synchronize()
        for (_, a), (name, b) in zip(self.events[:-1], self.events[1:]):
            self.out[name] = self.out.get(name, 0.0) + a.elapsed_time(b)


# ---------------------------------------------------------------------------------------------------------------------
def scan_number(name: str) -> int:
    """``scan9`` / ``9`` -> 9."""
    s = name.strip()
    digits = s[4:] if s.lower().startswith("scan") else s
    if not digits.isdigit():
        raise ValueError(f"cannot read a DTU scan number from {name!r}")
    return int(digits)


def scan_names(testlist: Optional[str], scans: Optional[str]) -> List[str]:
    if testlist:
        names = read_testlist(testlist)
    else:
        names = [s.strip() for s in scans.split(",") if s.strip()]
    return [f"scan{scan_number(s)}" for s in names]


def _mean(vals: Sequence[float]) -> float:
    return float(np.mean(vals)) if len(vals) else math.nan


def main(argv: Optional[Sequence[str]] = None) -> Dict[str, object]:
    ap = argparse.ArgumentParser(prog="python -m cds_mvsnet_amd.dtu_eval",
                                 description="DTU accuracy / completeness of fused point clouds, on the GPU")
    ap.add_argument("--datapath", required=True, help="the DTU 'MVS Data' folder (Points/stl, ObsMask)")
    ap.add_argument("--plydir", required=True, help="folder of the fused clouds (infer --fuse --outdir)")
    grp = ap.add_mutually_exclusive_group(required=True)
    grp.add_argument("--testlist", help="file with one scan per line (scan1, scan4, ...)")
    grp.add_argument("--scans", help="comma-separated scan numbers or names, e.g. 1,4,9")
    ap.add_argument("--ply", default="{scan}.ply", help="file name of a scan's cloud; {scan} = scan9, {n} = 9")
    ap.add_argument("--dst", type=float, default=0.2, help="thinning distance (mm)")
    ap.add_argument("--max-dist", type=float, default=20.0, help="outlier threshold (mm)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the thinning order")
    ap.add_argument("--json", help="write the per-scan and mean results here")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--sample_faces", nargs="?", type=float, const=0.0, default=None, metavar="SPACING",
                    help="the files are meshes: score the samples of their faces (sub-triangle centroids, edges of at most "
                         "SPACING, default --dst) instead of their vertices")
    args = ap.parse_args(argv)

    dev = torch.device(args.device)
    if dev.type != "cuda":
        raise SystemExit("dtu_eval runs on the GPU only (--device cuda[:N])")
    spacing = None
    if args.sample_faces is not None:
        spacing = args.sample_faces if args.sample_faces != 0.0 else args.dst
        if not (spacing > 0 and math.isfinite(spacing)):
            ap.error(f"--sample_faces must be positive, got {spacing}")
    names = scan_names(args.testlist, args.scans)
    jobs = []
    for name in names:                                       # resolve every file before the first scan is scored
        n = scan_number(name)
        ply = os.path.join(args.plydir, args.ply.format(scan=name, n=n))
        paths = dtu_scan_paths(args.datapath, n)
        for p in [ply] + list(paths.values()):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"{name}: {p} not found")
        jobs.append((name, n, ply))
    per_scan: Dict[str, Dict[str, object]] = {}
    with torch.cuda.device(dev):
        for name, n, ply in jobs:
            t0 = time.time()
            gt = load_dtu_scan(args.datapath, n)
            if spacing is None:
                pred, sampled = torch.from_numpy(read_ply_points(ply)).to(dev), None
            else:
                from .mesh import sample_file
                try:
                    out, sampled = sample_file(ply, spacing, dev)
                except ValueError as e:                          # a cloud, or a spacing too fine for the mesh
                    raise SystemExit(f"{name}: --sample_faces: {e}") from None
                pred = out["points"]
            r = evaluate(pred, gt, dst=args.dst, max_dist=args.max_dist, seed=args.seed)
            if sampled is not None:
                r.update(n_faces=sampled["faces"], n_sampled=sampled["points"])
            per_scan[name] = r
            print(f"{name}: acc {r['acc']:.4f}  comp {r['comp']:.4f}  overall {r['overall']:.4f}  "
                  f"({r['acc_n']} / {r['comp_n']} points, {time.time() - t0:.1f} s)"
                  + (f"  [{r['n_sampled']} samples of {r['n_faces']} faces]" if sampled is not None else ""), flush=True)
    acc = _mean([r["acc"] for r in per_scan.values()])
    comp = _mean([r["comp"] for r in per_scan.values()])
    mean = {"acc": acc, "comp": comp, "overall": (acc + comp) / 2.0}
    print(f"mean over {len(per_scan)} scans: acc {acc:.4f}  comp {comp:.4f}  overall {mean['overall']:.4f}")
    out = {"scans": per_scan, "mean": mean, "settings": {"dst": args.dst, "max_dist": args.max_dist, "seed": args.seed}}
    if spacing is not None:                                      # without the flag the output stays as it was
        out["settings"]["sample_faces"] = spacing
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
