"""Point-cloud primitives of the DTU and Tanks and Temples evaluations on the GPU: capped nearest-neighbour distances (with
or without the index of the neighbour), greedy thinning to a minimum spacing, voxel grouping with the merge of a fused cloud
to one attributed point per voxel (``csrc/cloud.hip``), statistical and radius outlier removal over k-nearest
distances and neighbour counts (``csrc/cloud_outlier.hip``), and a PLY vertex reader.

The hot paths are the HIP kernels of ``csrc/pointcloud.hip`` and ``csrc/registration.hip`` (``include/cds_mvsnet_hip.h``): a
sparse uniform grid with 64-bit cell keys and a hash table, queried one point per lane.  torch is used for device memory
and for the sort / unique / cumsum that lay the grid out.  Inputs must be float32 ROCm tensors; there is no CPU path.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops import _dev, _stream
from .ply import read_ply_points          # noqa: F401 (the evaluations import it from here)

Tensor = torch.Tensor

_MAX_AXIS = 1 << 21          # fine cells per axis that a key can address
_LOCAL_BITS = 9              # fine position inside its coarse cell (3 bits per axis)
_COARSE_FLAG = -(1 << 63)    # bit 63: coarse keys in the shared hash table


def _points(t: Tensor, name: str) -> Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name}: expected a [N,3] tensor, got {getattr(t, 'shape', type(t))}")
    _dev(t.contiguous(), name)                         # device, dtype and current-device checks
    if t.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"{name}: at most 2^31 - 1 points")
    return t.contiguous()


class PointGrid:
    """A sparse uniform grid over ``points`` [N,3] (float32, device) with fine cells of side ``cell``.

    Attributes (device tensors unless noted): ``pts`` [N,4] the points sorted by cell key (w = ``rank`` as int bits when
    given), ``perm`` [N] int64 sorted position -> input index, ``cell_keys`` [F] int64, ``cell_start`` [F+1] int32,
    ``coarse_start`` [C+1] int32, ``table_keys`` / ``table_vals`` the hash table, ``frame`` (CPU float32 [8]): origin,
    cell side, slop, cells per axis."""

    def __init__(self, points: Tensor, cell: Optional[float], rank: Optional[Tensor] = None,
                 thin_dist: Optional[float] = None):
        points = _points(points, "points")
        n = points.shape[0]
        if n == 0:
            raise ValueError("PointGrid: no points")
        lib = _lib.load()
        lo, hi = _bounds(points, "PointGrid")
        ext = float((hi - lo).max())
        self.slop = 2.0 ** -18 * (float(np.abs(np.concatenate([lo, hi])).max()) + ext) + 1e-30
        if thin_dist is not None:       # thinning: above min_dist plus the binning error, so 27 cells cover min_dist
            cell = thin_dist * (1.0 + 2.0 ** -10) + 4.0 * self.slop
        if not (cell is not None and cell > 0 and math.isfinite(cell)):
            raise ValueError(f"PointGrid: cell side must be positive, got {cell}")
        self.cell = max(float(cell), ext / (_MAX_AXIS - 64))
        origin = (lo - self.cell).astype(np.float32)
        dims = np.floor((hi - origin) / self.cell).astype(np.int64) + 3
        self.frame = torch.tensor([*origin.tolist(), self.cell, self.slop, *dims.tolist()], dtype=torch.float32)
        self.device = points.device
        stream = _stream(points)

        self.perm, self.cell_start, self.cell_keys, _ = _cell_layout(points, self.frame)
        ckeys, ccounts = torch.unique_consecutive(self.cell_keys >> _LOCAL_BITS, return_counts=True)
        self.coarse_start = _offsets(ccounts)
        all_keys = torch.cat([self.cell_keys, ckeys | _COARSE_FLAG])
        self.log2_slots = lib.cds_grid_hash_log2_slots(all_keys.numel())
        if self.log2_slots < 0:
            raise ValueError("PointGrid: too many cells")
        self.table_keys = torch.empty(1 << self.log2_slots, dtype=torch.int64, device=self.device)
        self.table_vals = torch.empty(1 << self.log2_slots, dtype=torch.int32, device=self.device)
        check(lib.cds_grid_hash_build(all_keys.data_ptr(), all_keys.numel(), self.cell_keys.numel(), self.table_keys.data_ptr(),
                                      self.table_vals.data_ptr(), self.log2_slots, stream), "cds_grid_hash_build")
        self.pts = torch.zeros((n, 4), dtype=torch.float32, device=self.device)
        self.pts[:, :3] = points[self.perm]
        if rank is not None:             # integer copy: rank bits must not pass through float arithmetic
            self.pts.view(torch.int32)[:, 3] = rank.to(self.device, torch.int32)[self.perm]
        self.n = n
        self.indexed = False            # True when the w lane holds each point's input index (index_grid)

    def keys(self, points: Tensor) -> Tensor:
        """Fine cell keys of arbitrary points in this grid's frame (coordinates clamped to the grid)."""
        return _cell_keys(points, self.frame)

    def query_order(self, query: Tensor) -> Tensor:
        """The permutation that puts ``query`` [M,3] into cell order (stable): a wave's lanes then search the same cells."""
        return torch.sort(self.keys(query), stable=True)[1]


def _bounds(points: Tensor, what: str):
    """(min, max) per axis of ``points`` as float64 numpy [3]; ValueError unless all are finite."""
    lo, hi = torch.aminmax(points, dim=0)
    lo, hi = lo.double().cpu().numpy(), hi.double().cpu().numpy()
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError(f"{what}: points must be finite")
    return lo, hi


def _cell_keys(points: Tensor, frame: Tensor) -> Tensor:
    keys = torch.empty(points.shape[0], dtype=torch.int64, device=points.device)
    check(_lib.load().cds_grid_keys_f32(points.data_ptr(), points.shape[0], frame.data_ptr(), keys.data_ptr(), _stream(points)),
          "cds_grid_keys_f32")
    return keys


def _offsets(counts: Tensor) -> Tensor:
    out = torch.zeros(counts.numel() + 1, dtype=torch.int32, device=counts.device)
    out[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return out


def _cell_layout(points: Tensor, frame: Tensor):
    """``points`` laid out by the cell keys of ``frame`` (CPU float32 [8]) -> (perm int64 [N]: the input indices sorted by key,
    stable; start int32 [V+1]: cell v holds perm[start[v]:start[v+1]]; keys int64 [V] ascending; counts int64 [V])."""
    skeys, perm = torch.sort(_cell_keys(points, frame), stable=True)
    ukeys, counts = torch.unique_consecutive(skeys, return_counts=True)
    return perm, _offsets(counts), ukeys, counts


def voxel_groups(points: Tensor, voxel: float, what: str = "voxel_groups"):
    """The occupied voxels of side ``voxel`` of ``points`` [N,3] (N >= 1, float32, device), Open3D's frame: origin
    ``o = float32(min - voxel / 2)`` per axis, voxel index ``floorf((p - o) / voxel)`` in fp32 (cds_grid_keys_f32), the grid's
    key packing.  -> (perm int64 [N]: the input indices sorted by key, stable; start int32 [V+1]: voxel v holds
    perm[start[v]:start[v+1]]; keys int64 [V] ascending; counts int64 [V]).  What cds_voxel_mean_f32 and cds_voxel_merge_f32
    take."""
    if not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError(f"{what}: voxel must be positive, got {voxel}")
    lo, hi = _bounds(points, what)
    origin = (lo - 0.5 * float(voxel)).astype(np.float32)
    dims = np.floor((hi - origin.astype(np.float64)) / float(np.float32(voxel))).astype(np.int64) + 2
    if int(dims.max()) > _MAX_AXIS:
        raise ValueError(f"{what}: {int(dims.max())} voxels along one axis, at most {_MAX_AXIS}")
    return _cell_layout(points, torch.tensor([*origin.tolist(), float(voxel), 0.0, *dims.tolist()], dtype=torch.float32))


def pack_colors(colors: Tensor) -> Tensor:
    """uint8 [N,3] (r, g, b) -> int32 [N] holding r | g << 8 | b << 16 (gipuma's packing; the bytes r g b 0 in memory)."""
    out = torch.zeros((colors.shape[0], 4), dtype=torch.uint8, device=colors.device)
    out[:, :3] = colors
    return out.view(torch.int32).reshape(-1)


def unpack_colors(packed: Tensor) -> Tensor:
    """The inverse of :func:`pack_colors`: int32 [N] -> uint8 [N,3]."""
    return packed.contiguous().view(torch.uint8).view(-1, 4)[:, :3].contiguous()


def merge_voxels(points: Tensor, colors: Tensor, voxel: float, normals: Optional[Tensor] = None, min_points: int = 1) -> dict:
    """One attributed point per occupied voxel of side ``voxel`` (cds_voxel_merge_f32): points [N,3] float32,
    colors uint8 [N,3] (or already packed, int32 [N]), normals [N,3] float32 or None, all on the device.  Position: the float64
    mean in input order, rounded once, the same bits as ``tt_eval.voxel_down_sample``; colour: the mean per channel rounded
    half up; normal: the float64 sum of the voxel's normals, normalised ((0,0,0) if they cancel); count: the voxel's points.
    Voxels with fewer than ``min_points`` points are dropped (isolated points are mostly outliers).  The output is in ascending
    voxel-key order, ``voxel_down_sample``'s frame and ordering.
    -> {"points" float32 [V,3], "colors" uint8 [V,3], "normals" float32 [V,3] | None, "counts" int32 [V]}."""
    points = _points(points, "points")
    n, dev = points.shape[0], points.device
    if not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError(f"merge_voxels: voxel must be positive, got {voxel}")
    if int(min_points) < 1:
        raise ValueError(f"merge_voxels: min_points must be >= 1, got {min_points}")
    if colors.dtype == torch.uint8 and tuple(colors.shape) == (n, 3):
        packed = pack_colors(colors.to(dev))
    elif colors.dtype == torch.int32 and tuple(colors.shape) == (n,):
        packed = colors.contiguous()
    else:
        raise ValueError(f"merge_voxels: colors must be uint8 [{n},3] or packed int32 [{n}], got {colors.dtype} "
                         f"{tuple(colors.shape)}")
    if not packed.is_cuda:
        raise RuntimeError("merge_voxels: colors must be a ROCm (cuda) tensor; there is no CPU fallback")
    if normals is not None:
        normals = _points(normals, "normals")
        if normals.shape[0] != n:
            raise ValueError(f"merge_voxels: {normals.shape[0]} normals for {n} points")
    if n == 0:
        return {"points": points.clone(), "colors": torch.zeros((0, 3), dtype=torch.uint8, device=dev),
                "normals": None if normals is None else normals.clone(), "counts": torch.zeros(0, dtype=torch.int32, device=dev)}
    perm, start, ukeys, _ = voxel_groups(points, voxel, "merge_voxels")
    v = ukeys.numel()
    out_p = torch.empty((v, 3), dtype=torch.float32, device=dev)
    out_c = torch.empty(v, dtype=torch.int32, device=dev)
    out_n = torch.empty((v, 3), dtype=torch.float32, device=dev) if normals is not None else None
    out_k = torch.empty(v, dtype=torch.int32, device=dev)
    check(_lib.load().cds_voxel_merge_f32(points.data_ptr(), packed.data_ptr(), normals.data_ptr() if normals is not None else None,
                                          n, perm.data_ptr(), start.data_ptr(), v, out_p.data_ptr(), out_c.data_ptr(),
                                          out_n.data_ptr() if out_n is not None else None, out_k.data_ptr(), _stream(points)),
          "cds_voxel_merge_f32")
    out_c = unpack_colors(out_c)
    if int(min_points) > 1:
        keep = out_k >= int(min_points)
        out_p, out_c, out_k = out_p[keep], out_c[keep], out_k[keep]
        out_n = out_n[keep] if out_n is not None else None
    return {"points": out_p, "colors": out_c, "normals": out_n, "counts": out_k}


def default_cell(points: Tensor) -> float:
    """Fine cell side for nearest-neighbour grids: twice the spacing of N points spread over the largest face of the
    bounding box (scanned clouds are surfaces; the coarse level absorbs a mismatch).  Only speed depends on it."""
    lo, hi = torch.aminmax(points, dim=0)
    e = sorted((hi - lo).double().cpu().tolist())
    area = max(e[1] * e[2], 1e-12)
    return max(2.0 * math.sqrt(area / max(points.shape[0], 1)), 1e-6 * max(e[2], 1.0))


def nearest_distance(query: Tensor, target: Tensor, max_dist: float, grid: Optional[PointGrid] = None,
                     cell: Optional[float] = None) -> Tensor:
    """For every query point [M,3] the distance to its nearest target point [N,3], capped at ``max_dist``:
    ``min(min_j |q - t_j|, max_dist)`` in fp32 with d2 = dx*dx + dy*dy + dz*dz (MaxDistCP.m, PointCompareMain.m:20-26;
    inside its block grid MaxDistCP returns exactly this, outside it max_dist).  An empty target gives max_dist everywhere.
    ``grid``: a PointGrid of ``target`` to reuse; ``cell``: its cell side (default: :func:`default_cell`)."""
    query = _points(query, "query")
    if not (max_dist >= 0):
        raise ValueError(f"nearest_distance: max_dist must be >= 0, got {max_dist}")
    m = query.shape[0]
    if target.shape[0] == 0 or m == 0:
        _points(target, "target")
        return torch.full((m,), float(max_dist), dtype=torch.float32, device=query.device)
    if grid is None:
        target = _points(target, "target")
        grid = PointGrid(target, cell if cell is not None else default_cell(target))
    order = grid.query_order(query)
    out = torch.empty(m, dtype=torch.float32, device=query.device)
    check(_lib.load().cds_nn_query_f32(query.data_ptr(), order.data_ptr(), m, *_grid_args(grid), float(max_dist), out.data_ptr(),
                                       _stream(query)), "cds_nn_query_f32")
    return out


def index_grid(target: Tensor, cell: Optional[float] = None) -> PointGrid:
    """A PointGrid of ``target`` whose w lane carries each point's input index (rank = arange(N)): what
    :func:`nearest_index` and the registration kernels search."""
    target = _points(target, "target")
    grid = PointGrid(target, cell if cell is not None else default_cell(target),
                     rank=torch.arange(target.shape[0], dtype=torch.int32, device=target.device))
    grid.indexed = True
    return grid


def _grid_args(grid: PointGrid):
    return (grid.pts.data_ptr(), grid.cell_start.data_ptr(), grid.cell_keys.data_ptr(), grid.coarse_start.data_ptr(),
            grid.table_keys.data_ptr(), grid.table_vals.data_ptr(), grid.log2_slots, grid.frame.data_ptr())


def nearest_index(query: Tensor, target: Tensor, max_dist: float, grid: Optional[PointGrid] = None,
                  cell: Optional[float] = None):
    """:func:`nearest_distance` that also says which target point was nearest -> (dist float32 [M], index int32 [M]).
    The smallest fp32 d2 = dx*dx + dy*dy + dz*dz wins and among equal d2 the lowest target index; it is accepted only if
    d2 < max_dist^2, otherwise dist = max_dist and index = -1 (also for an empty target).  ``grid``: an
    :func:`index_grid` of ``target`` to reuse."""
    query = _points(query, "query")
    if not (max_dist >= 0):
        raise ValueError(f"nearest_index: max_dist must be >= 0, got {max_dist}")
    m = query.shape[0]
    dist = torch.full((m,), float(max_dist), dtype=torch.float32, device=query.device)
    index = torch.full((m,), -1, dtype=torch.int32, device=query.device)
    if target.shape[0] == 0 or m == 0:
        _points(target, "target")
        return dist, index
    if grid is None:
        grid = index_grid(target, cell)
    elif not grid.indexed:
        raise ValueError("nearest_index: the grid must come from index_grid (its w lane holds the input indices)")
    order = grid.query_order(query)
    check(_lib.load().cds_nn_index_f32(query.data_ptr(), order.data_ptr(), m, *_grid_args(grid), float(max_dist),
                                       dist.data_ptr(), index.data_ptr(), _stream(query)), "cds_nn_index_f32")
    return dist, index


KNN_MAX_K = 64               # CDS_KNN_MAX_K
_STAT_CHUNK = 4096           # CDS_STAT_CHUNK


def knn_cell(cell: float, k: int) -> float:
    """Fine cell side of a grid searched for k neighbours, from the :func:`default_cell` of the cloud: the 27 cells around a
    query should hold most of its k nearest (measured, profiles/cloud_outliers.md).  Only speed depends on it."""
    return cell * (1.5 if k <= 12 else 2.0)


def knn_mean_distance(query: Tensor, target: Tensor, k: int, max_dist: float = math.inf, grid: Optional[PointGrid] = None,
                      cell: Optional[float] = None, want_kth: bool = False):
    """For every query point [M,3] the mean distance to its ``k`` nearest target points [N,3] -> float64 [M]
    (cds_knn_mean_f64).  d2 = dx*dx + dy*dy + dz*dz in fp32; a query that is a target point counts itself at 0.
    The k smallest d2 below ``max_dist``^2 (fp32) give the terms sqrt(d2) in fp64, summed in ascending order; each of the k
    terms that is missing counts as ``max_dist``; the sum is divided by k.  ``max_dist = inf``: the exact k nearest, min(k, N)
    terms (the walk then ends only when the grid is exhausted: an isolated query visits all of it).  ``want_kth``: also the
    distance to the k-th neighbour, float32 [M] (``max_dist`` when a term is missing).  ``grid``: a PointGrid of ``target`` to
    reuse; ``cell``: its cell side (default: :func:`knn_cell` of :func:`default_cell`)."""
    query = _points(query, "query")
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"knn_mean_distance: k must be in 1..{KNN_MAX_K}, got {k}")
    if not (max_dist >= 0):
        raise ValueError(f"knn_mean_distance: max_dist must be >= 0, got {max_dist}")
    m = query.shape[0]
    if grid is None:
        target = _points(target, "target")
        if target.shape[0] == 0:
            raise ValueError("knn_mean_distance: no target points")
        grid = PointGrid(target, cell if cell is not None else knn_cell(default_cell(target), k))
    mean = torch.empty(m, dtype=torch.float64, device=query.device)
    kth = torch.empty(m, dtype=torch.float32, device=query.device) if want_kth else None
    if m > 0:
        order = grid.query_order(query)
        check(_lib.load().cds_knn_mean_f64(query.data_ptr(), order.data_ptr(), m, *_grid_args(grid), k, float(max_dist),
                                           mean.data_ptr(), kth.data_ptr() if want_kth else None, _stream(query)),
              "cds_knn_mean_f64")
    return (mean, kth) if want_kth else mean


def radius_count(query: Tensor, target: Tensor, radius: float, cap: int, grid: Optional[PointGrid] = None) -> Tensor:
    """For every query point [M,3] the number of target points [N,3] with d2 <= ``radius``^2 (fp32, d2 as everywhere here),
    counted up to ``cap`` -> int32 [M] (cds_radius_count_f32).  A query that is a target point counts itself.  ``grid``: a
    PointGrid of ``target`` whose cell side is at least ``radius``; by default one is built with the cell of
    :func:`reduce_points`, just above ``radius``."""
    query = _points(query, "query")
    f = float(np.float32(radius))
    if not (f > 0 and math.isfinite(f)):
        raise ValueError(f"radius_count: radius must be positive, got {radius}")
    if int(cap) < 1:
        raise ValueError(f"radius_count: cap must be >= 1, got {cap}")
    m = query.shape[0]
    out = torch.zeros(m, dtype=torch.int32, device=query.device)
    if grid is None:
        target = _points(target, "target")
        if target.shape[0] == 0:
            return out
        grid = PointGrid(target, None, thin_dist=f)
    if float(grid.frame[3]) < f:
        raise ValueError(f"radius_count: the grid's cell side {float(grid.frame[3])} is below the radius {f}")
    if m > 0:
        order = grid.query_order(query)
        check(_lib.load().cds_radius_count_f32(query.data_ptr(), order.data_ptr(), m, *_grid_args(grid), f,
                                               min(int(cap), 2 ** 31 - 1), out.data_ptr(), _stream(query)),
              "cds_radius_count_f32")
    return out


def outlier_stats(x: Tensor) -> Tensor:
    """(mean, sample standard deviation) of ``x`` float64 [N >= 1] on the device -> float64 [2] on the device, summed in the
    fixed order of cds_outlier_stats_f64: one value for the same input, whatever the machine does."""
    if x.dtype != torch.float64 or x.dim() != 1 or not x.is_cuda or x.numel() < 1:
        raise ValueError("outlier_stats: expected a non-empty float64 vector on the device")
    x = x.contiguous()
    chunks = (x.numel() + _STAT_CHUNK - 1) // _STAT_CHUNK
    ws = torch.empty(chunks, dtype=torch.float64, device=x.device)
    out = torch.empty(2, dtype=torch.float64, device=x.device)
    check(_lib.load().cds_outlier_stats_f64(x.data_ptr(), x.numel(), ws.data_ptr(), chunks, out.data_ptr(), _stream(x)),
          "cds_outlier_stats_f64")
    return out


def check_outlier_args(nb_neighbors: int = 0, std_ratio: float = 2.0, radius: float = 0.0, min_neighbors: int = 0,
                       max_dist: Optional[float] = None) -> None:
    """The argument rules of :func:`remove_outliers` (ValueError); the command lines call it before any work is done."""
    if not 0 <= int(nb_neighbors) <= KNN_MAX_K - 1:
        raise ValueError(f"remove_outliers: nb_neighbors must be in 0..{KNN_MAX_K - 1} (k = nb_neighbors + 1 <= {KNN_MAX_K}), "
                         f"got {nb_neighbors}")
    if not (std_ratio >= 0 and math.isfinite(std_ratio)):
        raise ValueError(f"remove_outliers: std_ratio must be finite and >= 0, got {std_ratio}")
    if not (radius >= 0 and math.isfinite(radius)):
        raise ValueError(f"remove_outliers: radius must be finite and >= 0, got {radius}")
    if int(min_neighbors) < 0:
        raise ValueError(f"remove_outliers: min_neighbors must be >= 0, got {min_neighbors}")
    if radius > 0 and int(min_neighbors) < 1:
        raise ValueError("remove_outliers: radius needs min_neighbors >= 1")
    if int(min_neighbors) > 0 and not radius > 0:
        raise ValueError("remove_outliers: min_neighbors belongs to the radius filter, give radius > 0")
    if max_dist is not None and not (max_dist > 0):
        raise ValueError(f"remove_outliers: max_dist must be positive, got {max_dist}")
    if max_dist is not None and int(nb_neighbors) == 0:
        raise ValueError("remove_outliers: max_dist belongs to the statistical filter, give nb_neighbors > 0")


def remove_outliers(points: Tensor, nb_neighbors: int = 0, std_ratio: float = 2.0, radius: float = 0.0,
                    min_neighbors: int = 0, max_dist: Optional[float] = None, info: Optional[dict] = None) -> Tensor:
    """Keep mask bool [N] of the two standard outlier filters, both judged on the input cloud [N,3]:

    statistical (``nb_neighbors`` > 0): m_i = :func:`knn_mean_distance` of the cloud against itself with
    k = nb_neighbors + 1 (the point itself at distance 0 plus nb_neighbors others); mu, sigma = :func:`outlier_stats` of m;
    kept iff m_i <= T = mu + std_ratio * sigma (fp64).  ``max_dist`` caps every neighbour distance (default
    16 * :func:`default_cell`): it bounds the search of an isolated point, and such a point enters mu and sigma with the cap.
    radius (``radius`` > 0): kept iff at least ``min_neighbors`` other points lie within ``radius``
    (:func:`radius_count` with cap = min_neighbors + 1, the point itself included).
    With both, a point must pass both.  ``info`` receives mu, sigma, threshold (None without the statistical filter),
    removed_statistical, removed_radius."""
    points = _points(points, "points")
    check_outlier_args(nb_neighbors, std_ratio, radius, min_neighbors, max_dist)
    n = points.shape[0]
    keep = torch.ones(n, dtype=torch.bool, device=points.device)
    stats = {"mu": None, "sigma": None, "threshold": None, "removed_statistical": 0, "removed_radius": 0}
    if n > 0 and int(nb_neighbors) > 0:
        cell = default_cell(points)
        cap = 16.0 * cell if max_dist is None else float(max_dist)
        mean = knn_mean_distance(points, points, int(nb_neighbors) + 1, cap, cell=knn_cell(cell, int(nb_neighbors) + 1))
        mu, sigma = outlier_stats(mean).cpu().tolist()
        threshold = mu + float(std_ratio) * sigma
        ok = mean <= threshold
        stats.update(mu=mu, sigma=sigma, threshold=threshold, removed_statistical=n - int(ok.sum()))
        keep &= ok
    if n > 0 and radius > 0:
        ok = radius_count(points, points, radius, int(min_neighbors) + 1) >= int(min_neighbors) + 1
        stats["removed_radius"] = n - int(ok.sum())
        keep &= ok
    if info is not None:
        info.update(stats)
    return keep


def thinning_order(n: int, seed: int = 0) -> Tensor:
    """The visiting order of :func:`reduce_points`: ``torch.randperm`` from a CPU generator seeded with ``seed``, the same on
    every machine (MATLAB's ``randperm`` of reducePts_haa.m:9 cannot be reproduced)."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))


def reduce_points(points: Tensor, min_dist: float, order: Optional[Tensor] = None, seed: int = 0,
                  check_every: int = 4, info: Optional[dict] = None) -> Tensor:
    """Greedy thinning of reducePts_haa.m (PointCompareMain.m:7): visit the points in ``order`` (a permutation of range(N);
    default :func:`thinning_order` of ``seed``); a point still kept removes every other point within ``min_dist``
    (d2 <= min_dist^2 in fp32).  -> keep mask bool[N] on the points' device, the greedy maximal independent set in that
    order.  Computed in parallel rounds (cds_thin_round_f32) that converge to the same set bit for bit; the host reads
    the count of undecided points every ``check_every`` rounds.  ``info``: a dict that receives the number of rounds."""
    points = _points(points, "points")
    n = points.shape[0]
    if not (min_dist > 0 and math.isfinite(min_dist)):
        raise ValueError(f"reduce_points: min_dist must be positive, got {min_dist}")
    if n == 0:
        return torch.zeros(0, dtype=torch.bool, device=points.device)
    if order is None:
        order = thinning_order(n, seed).to(points.device)
    else:
        order = torch.as_tensor(order).to(points.device, torch.int64).reshape(-1)
        if order.numel() != n or not bool(((order >= 0) & (order < n)).all()) or \
                not bool((torch.bincount(order, minlength=n) == 1).all()):
            raise ValueError("reduce_points: order must be a permutation of range(N)")
    rank = torch.empty(n, dtype=torch.int32, device=points.device)
    rank[order] = torch.arange(n, dtype=torch.int32, device=points.device)
    lib = _lib.load()
    f = float(np.float32(min_dist))
    grid = PointGrid(points, None, rank=rank, thin_dist=f)
    if grid.cell < f:
        raise ValueError("reduce_points: cell side below min_dist")
    state = torch.zeros(n, dtype=torch.uint8, device=points.device)
    counter = torch.zeros(1, dtype=torch.int32, device=points.device)
    stream = _stream(points)
    pts, cell_start, _, _, *table = _grid_args(grid)         # a thinning round reads the fine level only
    rounds = 0
    while True:
        counter.zero_()
        for k in range(check_every):
            check(lib.cds_thin_round_f32(pts, cell_start, n, *table, f, state.data_ptr(),
                                         counter.data_ptr() if k == check_every - 1 else None, stream), "cds_thin_round_f32")
        rounds += check_every
        if int(counter.item()) == 0:
            break
        if rounds > n + check_every:                    # each round decides the lowest-rank undecided point
            raise RuntimeError("reduce_points: thinning rounds did not converge")
    keep = torch.empty(n, dtype=torch.bool, device=points.device)
    keep[grid.perm] = state == 1
    if info is not None:
        info["rounds"] = rounds
    return keep
