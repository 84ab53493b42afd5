"""A triangle mesh from the fused depth maps of a scan, on the GPU (the rule is in include/cds_mvsnet_hip.h).

The fused depth map, consistency mask, camera and image of every reference view, all on the device at the end of
:func:`cds_mvsnet_amd.fusion.filter_depth`, are integrated into a sparse truncated signed distance volume (blocks of 8x8x8
lattice points around the kept points) and the zero level set is extracted as the triangles of the six Freudenthal tetrahedra
of every cube: welded vertices, consistent winding, colours, a fixed order.  The hot paths are the kernels of ``csrc/tsdf.hip``
(``cds_tsdf_integrate_f32``, ``cds_tsdf_classify``, ``cds_tsdf_emit``); torch does the keys, unique and prefix sums that lay
the blocks out.  There is no CPU path.

    python -m cds_mvsnet_amd.mesh --testpath <scenes> --outdir <out> --testlist <list> --mesh_voxel SIZE [--mesh_trunc T]
        [--mesh_min_weight 2] [--mesh_min_component N] [--mesh_keep_largest K] [--mesh_simplify CELL]
        [--mesh_simplify_placement quadric|mean] [--mesh_fill_holes N] [--mesh_smooth ITER] [--mesh_smooth_lambda 0.5] [--mesh_smooth_mu -0.53]
        [--mesh_smooth_max_move D] [--mesh_sample SPACING] [--mesh_weight one|angle|conf|angle_conf] [--mesh_interp]
        [--mesh_interp_jump 0.05] [--filter_method normal|dynamic] [--conf 0,0,0] [--thres_disp 1.0] [--thres_view 3]
        [--dyn_dist_base 0.25] [--dyn_rel_base 0.000769] [--dyn_views 2,10]

fuses the saved depth maps of ``<out>/<scan>/`` as ``python -m cds_mvsnet_amd.fusion`` does and writes
``<out>/<scan>_mesh.ply``.  ``infer ... --fuse --mesh_voxel SIZE`` writes cloud and mesh from one fusion pass.

``--mesh_min_component N`` / ``--mesh_keep_largest K`` drop the small connected components of the mesh before it is written
(the kernels of ``csrc/mesh_clean.hip``: a union-find over the vertices, face counts per component, compaction).

    python -m cds_mvsnet_amd.mesh --from_mesh "<out>/{scan}_mesh.ply" --mesh_min_component N [--mesh_keep_largest K]
        --outdir <out> --testlist <list>

cleans saved meshes in place, without the fusion.

``--mesh_simplify CELL`` simplifies the mesh before it is written, after the clean-up (the kernels of
``csrc/mesh_simplify.hip``): the vertices of a cell of side CELL, the cells of ``--merge_voxel``, become one vertex at the
regularised minimiser of its faces' quadric error (``--mesh_simplify_placement mean``: at their mean), and the faces that
collapse or repeat are dropped.  ``--from_mesh FILE --mesh_simplify CELL`` does it to a saved mesh.

``--mesh_smooth ITER`` smooths the mesh after the clean-up and before the simplification (the kernels of
``csrc/mesh_smooth.hip``): ITER iterations of the lambda|mu filter move every vertex towards the mean of its neighbours and back,
which takes the noise of the depth maps and the staircase of the tetrahedra out of the surface without shrinking it; faces,
colours and counts stay as they are.  ``--mesh_smooth_max_move D`` keeps every vertex within D of where it was.
``--from_mesh FILE --mesh_smooth ITER`` does it to a saved mesh.

``--mesh_fill_holes N`` closes the holes of the mesh whose rim has at most N border edges, after the clean-up and before the
smoothing (the kernels of ``csrc/mesh_fill.hip``): a hole of three edges gets one face, a larger one a new vertex
at the mean of its rim and a fan of faces around it, oriented as the surface around the hole.  The rows of the input stay bit for
bit; the fan is flat, so ``--mesh_smooth`` after it fairs the cap.  ``--from_mesh FILE --mesh_fill_holes N`` does it to a saved mesh.

``--mesh_sample SPACING`` also writes ``<out>/<scan>_surface.ply``, the surface of the mesh written as a cloud (the
kernels of ``csrc/mesh_sample.hip``): every face is cut into n^2 congruent sub-triangles with edges of at most SPACING and the
centroid of each becomes a point, so that every point of the surface lies within 2/3 SPACING of one.  It is what
``dtu_eval --sample_faces`` and ``tt_eval --sample_faces`` score instead of a mesh's vertices (:func:`sample_mesh`).

``--mesh_weight angle|conf|angle_conf`` weighs every kept pixel by the cosine between its viewing ray and the normal of its depth
map, by its confidence, or by both, and ``--mesh_interp`` interpolates the depth between pixels where they belong to one surface
(``cds_tsdf_view_weights``, ``cds_tsdf_integrate_w_f32``): a pixel seen at a grazing angle no longer pulls the
surface as hard as one seen head-on.  Without them nothing of that runs and the mesh is what it was.
"""
from __future__ import annotations

import argparse
import math
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check
from .mvs_io import read_testlist
from .ply import read_mesh_ply, write_mesh_ply, write_ply

Tensor = torch.Tensor

MAX_CELLS = 1 << 26            # cells of the dense block table (CDS_TSDF_MAX_CELLS): 256 MiB of int32
MAX_CHUNK = 32                 # views per launch the kernel takes (CDS_TSDF_MAX_CHUNK)
CHUNK_VIEWS = 32               # views per launch of TsdfVolume.integrate (profiles/tsdf_mesh.md: 3.5 x faster than 1)
WEIGHT_MODES = ("one", "angle", "conf", "angle_conf")   # what a pixel weighs in the integration
MAX_ROUNDS = 64                # hook passes of the component labelling before it gives up (CDS_MESH_CC_MAX_ROUNDS)
SMOOTH_KEYS = ("smooth", "smooth_lambda", "smooth_mu", "smooth_max_move")   # the smoothing arguments of mesh_scan and clean_file
PLACEMENTS = ("quadric", "mean")   # where simplify_mesh puts a cluster's vertex
MAX_SAMPLE_N = 1 << 15         # subdivisions per edge sample_mesh takes (CDS_MESH_SAMPLE_MAX_N): n^2 and the weights fit an int32
MAX_SAMPLES = 1 << 28          # points sample_mesh makes unless told otherwise: 19 bytes each, 4.75 GiB
MAX_SMOOTH = 1000              # iterations smooth_mesh takes
ADJ_SMALL = 64                 # entries of a vertex's segment that cds_mesh_adj_finish sorts itself (CDS_MESH_ADJ_SMALL)
ADJ_BOUNDARY, ADJ_ISOLATED = 1, 2   # the flag bits of cds_mesh_adj_finish
MAX_FILL_EDGES = 4096          # border edges of the largest hole fill_holes takes (CDS_MESH_FILL_MAX_EDGES): one thread walks a loop
PACK_BITS = 21                 # three cluster numbers of at most this many bits make one sort key of a face's identity


def _positive(value, name: str, what: str = "") -> float:
    """-> value as a float; ValueError "[what: ]name must be positive" unless it is finite and > 0."""
    try:
        size = float(value)
    except (TypeError, ValueError):
        size = math.nan
    if not (size > 0 and math.isfinite(size)):
        raise ValueError(f"{what + ': ' if what else ''}{name} must be positive, got {value}")
    return size


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _empty_mesh(dev, nv: int = 0, nf: int = 0) -> Dict[str, Tensor]:
    """A mesh dict of nv and nf rows to be written; the empty mesh by default."""
    return {"vertices": torch.empty((nv, 3), dtype=torch.float32, device=dev),
            "colors": torch.empty((nv, 3), dtype=torch.uint8, device=dev), "faces": torch.empty((nf, 3), dtype=torch.int32, device=dev)}


def check_voxel(voxel, trunc=None, what: str = "mesh"):
    """-> (voxel, trunc) as floats; trunc defaults to 4 voxels.  ValueError unless voxel > 0 and voxel <= trunc <= 8 voxel."""
    voxel = _positive(voxel, "voxel", what)
    trunc = 4.0 * voxel if trunc is None else float(trunc)
    if not (voxel <= trunc <= 8.0 * voxel):
        raise ValueError(f"{what}: trunc must lie in [voxel, 8 voxel] = [{voxel}, {8.0 * voxel}], got {trunc} (the band of +-trunc "
                         "along a ray must stay inside the blocks next to its point)")
    return voxel, trunc


def check_grid(nb, voxel: float, what: str = "mesh") -> None:
    cells = int(nb[0]) * int(nb[1]) * int(nb[2])
    if cells > MAX_CELLS:
        raise ValueError(f"{what}: a voxel of {voxel} gives a grid of {int(nb[0])} x {int(nb[1])} x {int(nb[2])} = {cells} blocks, "
                         f"at most {MAX_CELLS}: raise --mesh_voxel")


class TsdfVolume:
    """The sparse volume of one scan.  ``points`` [N,3] float32 on the device: the kept points of every view; they fix the frame
    (origin, blocks per axis) and the allocated blocks (a block that holds a point, and its 26 neighbours inside the grid).

    Attributes: ``voxel``, ``trunc``, ``origin`` (float64 numpy [3]), ``nb`` (int64 numpy [3]: blocks per axis x, y, z),
    ``keys`` int32 [NB] ascending, ``table`` int32 [nbz,nby,nbx] (-1: no block), ``sum`` float32 [NB,512], ``n`` / ``nc``
    int32 [NB,512], ``rgb`` int32 [3,NB,512]; ``wn`` int32 [NB,512], the sum of the weights, once views came with weights
    (DESIGN §1.14), else None."""

    def __init__(self, points: Tensor, voxel: float, trunc: Optional[float] = None):
        voxel, trunc = check_voxel(voxel, trunc, "TsdfVolume")
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
            raise ValueError(f"TsdfVolume: points must be a float32 [N,3] tensor, got {getattr(points, 'shape', type(points))}")
        if not points.is_cuda:
            raise RuntimeError("TsdfVolume: points must be a ROCm (cuda) tensor; there is no CPU fallback")
        if points.shape[0] == 0:
            self._setup(np.zeros(3), voxel, trunc, np.ones(3, np.int64), torch.zeros(0, dtype=torch.int64, device=points.device))
            return
        lo, hi = torch.aminmax(points, dim=0)
        lo, hi = lo.double().cpu().numpy(), hi.double().cpu().numpy()
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError("TsdfVolume: points must be finite")
        b = 8.0 * voxel
        origin = (np.floor(lo / b) - 1.0) * b
        nbf = np.floor((hi - origin) / b) + 2.0
        if not (np.isfinite(origin).all() and float(nbf.max()) < 2.0 ** 31):
            raise ValueError(f"TsdfVolume: a voxel of {voxel} is too small for this scan: raise --mesh_voxel")
        nb = nbf.astype(np.int64)
        check_grid(nb, voxel, "TsdfVolume")
        dev = points.device
        bi = torch.floor((points.double() - torch.from_numpy(origin).to(dev)) / b).long()
        own = torch.unique((bi[:, 2] * int(nb[1]) + bi[:, 1]) * int(nb[0]) + bi[:, 0])
        ox, oy, oz = own % int(nb[0]), (own // int(nb[0])) % int(nb[1]), own // (int(nb[0]) * int(nb[1]))
        near = []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    x, y, z = ox + dx, oy + dy, oz + dz
                    ok = (x >= 0) & (x < int(nb[0])) & (y >= 0) & (y < int(nb[1])) & (z >= 0) & (z < int(nb[2]))
                    near.append(((z * int(nb[1]) + y) * int(nb[0]) + x)[ok])
        self._setup(origin, voxel, trunc, nb, torch.unique(torch.cat(near)))

    @classmethod
    def from_blocks(cls, origin, voxel: float, trunc: float, nb, keys, device="cuda") -> "TsdfVolume":
        """A volume with a given frame and block set (``keys``: block keys (bz nby + by) nbx + bx, any order), zeroed."""
        voxel, trunc = check_voxel(voxel, trunc, "TsdfVolume")
        nb = np.asarray(nb, np.int64).reshape(3)
        if int(nb.min()) < 1:
            raise ValueError(f"TsdfVolume: blocks per axis must be >= 1, got {nb.tolist()}")
        check_grid(nb, voxel, "TsdfVolume")
        keys = torch.unique(torch.as_tensor(np.asarray(keys, np.int64)).to(device))
        if keys.numel() and (int(keys[0]) < 0 or int(keys[-1]) >= int(nb[0]) * int(nb[1]) * int(nb[2])):
            raise ValueError("TsdfVolume: block keys outside the grid")
        self = cls.__new__(cls)
        self._setup(np.asarray(origin, np.float64).reshape(3), voxel, trunc, nb, keys)
        return self

    def _setup(self, origin, voxel, trunc, nb, keys64: Tensor) -> None:
        dev = keys64.device
        self.voxel, self.trunc, self.origin, self.nb, self.device = voxel, trunc, origin, nb, dev
        self.n_blocks = k = int(keys64.numel())
        self.keys = keys64.to(torch.int32)
        self.table = torch.full((int(nb[2]), int(nb[1]), int(nb[0])), -1, dtype=torch.int32, device=dev)
        self.table.view(-1)[keys64] = torch.arange(k, dtype=torch.int32, device=dev)
        self.sum = torch.zeros((k, 512), dtype=torch.float32, device=dev)
        self.n = torch.zeros((k, 512), dtype=torch.int32, device=dev)
        self.nc = torch.zeros((k, 512), dtype=torch.int32, device=dev)
        self.rgb = torch.zeros((3, k, 512), dtype=torch.int32, device=dev)
        self.wn = None                       # int32 [NB,512], the sum of the weights: allocated by the first weighted integrate
        self._weighted = None                # whether the views so far came with weights; None before the first
        self._frame = torch.tensor([*origin.tolist(), voxel], dtype=torch.float64)          # host arguments of the kernels
        self._dims = torch.tensor(nb.tolist(), dtype=torch.int32)

    def integrate(self, depths: Tensor, masks: Tensor, images: Tensor, cams: Tensor, chunk: int = CHUNK_VIEWS,
                  weights: Optional[Tensor] = None, interp: bool = False, interp_jump: float = 0.05) -> None:
        """Add views in the order given: depths [V,h,w] float32, masks [V,h,w] (bool, uint8 or float: non-zero keeps the
        pixel), images [V,h,w,3] uint8, all on the volume's device; cams [V,2,4,4] float32 (extrinsic; intrinsic in [:3,:3]),
        any device.  ``chunk`` views go into one launch (1..32); the result does not depend on it.

        ``weights`` uint8 [V,h,w] on the volume's device (:func:`view_weights`): a pixel counts that many times in ``sum`` and in
        ``wn``, the weight sum that :meth:`extract` then divides by, and not at all at 0; every call on one volume comes with
        weights or none does (ValueError).  ``interp``: the depth is interpolated in inverse depth between the four pixel centres
        around the projection where all four are kept and within ``interp_jump`` (relative) of each other, and is the nearest
        pixel's elsewhere.  Both are the rule of DESIGN §1.14 (``cds_tsdf_integrate_w_f32``); with neither, the call is what it
        was without them."""
        if not (1 <= int(chunk) <= MAX_CHUNK):
            raise ValueError(f"TsdfVolume.integrate: chunk must lie in 1..{MAX_CHUNK}, got {chunk}")
        if interp:
            interp_jump = _positive(interp_jump, "interp_jump", "TsdfVolume.integrate")
        if depths.dim() != 3 or depths.dtype != torch.float32:
            raise ValueError(f"TsdfVolume.integrate: depths must be float32 [V,h,w], got {depths.dtype} {tuple(depths.shape)}")
        v, h, w = depths.shape
        if tuple(masks.shape) != (v, h, w) or tuple(images.shape) != (v, h, w, 3) or images.dtype != torch.uint8 or \
                tuple(cams.shape) != (v, 2, 4, 4):
            raise ValueError(f"TsdfVolume.integrate: for depths {tuple(depths.shape)} masks must be [V,h,w], images uint8 [V,h,w,3] "
                             f"and cams [V,2,4,4]; got {tuple(masks.shape)}, {images.dtype} {tuple(images.shape)}, {tuple(cams.shape)}")
        if weights is not None and (tuple(weights.shape) != (v, h, w) or weights.dtype != torch.uint8):
            raise ValueError(f"TsdfVolume.integrate: weights must be uint8 {(v, h, w)}, got {weights.dtype} {tuple(weights.shape)}")
        for t, name in ((depths, "depths"), (masks, "masks"), (images, "images"), (weights, "weights")):
            if t is not None and t.device != self.device:
                raise RuntimeError(f"TsdfVolume.integrate: {name} must be on {self.device}; there is no CPU fallback")
        if self._weighted is not None and self._weighted != (weights is not None):
            raise ValueError("TsdfVolume.integrate: this volume holds views " + ("with" if self._weighted else "without") +
                             " weights; weighted and unweighted views do not mix in one volume")
        if v == 0 or self.n_blocks == 0:
            return
        self._weighted = weights is not None
        if weights is not None:
            weights = weights.contiguous()
            if self.wn is None:
                self.wn = torch.zeros((self.n_blocks, 512), dtype=torch.int32, device=self.device)
        depths, images = depths.contiguous(), images.contiguous()
        masks = (masks != 0).to(torch.uint8).contiguous()
        cam = cams.detach().to(torch.float32).to(self.device).double()
        ok = (masks != 0) & torch.isfinite(depths) & (depths > 0)
        far = torch.where(ok, depths, torch.full_like(depths, -math.inf)).flatten(1).amax(1).double()
        tab = torch.zeros((v, 24), dtype=torch.float64, device=self.device)
        tab[:, 0:9] = cam[:, 0, :3, :3].reshape(v, 9)
        tab[:, 9:12] = cam[:, 0, :3, 3]
        tab[:, 12:21] = cam[:, 1, :3, :3].reshape(v, 9)
        tab[:, 21] = far
        lib, hw = _lib.load(), h * w
        with torch.cuda.device(self.device):
            for v0 in range(0, v, int(chunk)):
                nv = min(int(chunk), v - v0)
                args = (self.keys.data_ptr(), self.n_blocks, self._frame.data_ptr(), self._dims.data_ptr(), self.trunc,
                        depths.data_ptr() + 4 * v0 * hw, masks.data_ptr() + v0 * hw, images.data_ptr() + 3 * v0 * hw,
                        tab.data_ptr() + 8 * 24 * v0, nv, h, w, self.sum.data_ptr(), self.n.data_ptr(), self.nc.data_ptr(),
                        self.rgb.data_ptr())
                if weights is None and not interp:
                    check(lib.cds_tsdf_integrate_f32(*args, _stream(self.device)), "cds_tsdf_integrate_f32")
                else:
                    check(lib.cds_tsdf_integrate_w_f32(*args, weights.data_ptr() + v0 * hw if weights is not None else None,
                                                       1 if interp else 0, float(interp_jump),
                                                       self.wn.data_ptr() if weights is not None else None, _stream(self.device)),
                          "cds_tsdf_integrate_w_f32")

    def extract(self, min_weight: int = 2) -> Dict[str, Tensor]:
        """The zero level set over the cubes whose eight corners were seen at least ``min_weight`` times
        -> {"vertices" float32 [V,3], "colors" uint8 [V,3], "faces" int32 [F,3]} on the device."""
        if int(min_weight) < 1:
            raise ValueError(f"TsdfVolume.extract: min_weight must be >= 1, got {min_weight}")
        dev, k = self.device, self.n_blocks
        if k == 0:
            return _empty_mesh(dev)
        lib = _lib.load()
        vmask = torch.empty((k, 512), dtype=torch.uint8, device=dev)
        tcount = torch.empty((k, 512), dtype=torch.uint8, device=dev)
        bv = torch.empty(k, dtype=torch.int32, device=dev)
        bt = torch.empty(k, dtype=torch.int32, device=dev)
        frame = (self._frame.data_ptr(), self._dims.data_ptr())
        with torch.cuda.device(dev):
            check(lib.cds_tsdf_classify(self.keys.data_ptr(), self.table.data_ptr(), k, *frame, self.sum.data_ptr(), self.n.data_ptr(),
                                        int(min_weight), vmask.data_ptr(), tcount.data_ptr(), bv.data_ptr(), bt.data_ptr(),
                                        _stream(self.device)), "cds_tsdf_classify")
            ends = torch.stack([torch.cumsum(bv, 0, dtype=torch.int64), torch.cumsum(bt, 0, dtype=torch.int64)])
            nv, nf = (int(x) for x in ends[:, -1].cpu())
            if nv >= 2 ** 31 or nf >= 2 ** 31:
                raise ValueError(f"TsdfVolume.extract: {nv} vertices and {nf} faces, at most 2^31 - 1 each: raise --mesh_voxel")
            if nv == 0:
                return _empty_mesh(dev)
            vfirst = (ends[0] - bv).to(torch.int32)
            tfirst = (ends[1] - bt).to(torch.int32)
            vstart = torch.empty((k, 512), dtype=torch.int32, device=dev)
            out = _empty_mesh(dev, nv, nf)
            denom = self.wn if self.wn is not None else self.n                 # a weighted volume's distance is sum / wn (§1.14)
            check(lib.cds_tsdf_emit(self.keys.data_ptr(), self.table.data_ptr(), k, *frame, self.sum.data_ptr(), denom.data_ptr(),
                                    self.nc.data_ptr(), self.rgb.data_ptr(), vmask.data_ptr(), tcount.data_ptr(), vfirst.data_ptr(),
                                    tfirst.data_ptr(), nv, nf, vstart.data_ptr(), out["vertices"].data_ptr(), out["colors"].data_ptr(),
                                    out["faces"].data_ptr() if nf else None, _stream(self.device)), "cds_tsdf_emit")
        return out


def view_weights(depth: Tensor, mask: Tensor, cam: Tensor, conf: Optional[Tensor] = None, mode: str = "angle", radius: int = 2,
                 jump: float = 0.01, min_pts: int = 6) -> Tensor:
    """The weight map of one view for :meth:`TsdfVolume.integrate` (``cds_tsdf_view_weights``): depth float32
    [h,w] and mask [h,w] (bool, uint8 or float: non-zero keeps the pixel) on a ROCm device, cam [2,4,4] (extrinsic; intrinsic in
    [:3,:3]; any device), conf [h,w] floating point on the device or None -> uint8 [h,w] on the device: 0 where the pixel is not kept,
    else 1..255.  ``mode``: "angle", 255 times the cosine between the viewing ray and the normal of the depth map there
    (:func:`ops.depth_normals` over the kept pixels with ``radius``, ``jump``, ``min_pts``; 1 where there is no normal or it
    faces away); "conf", 255 times ``conf`` clamped to [0, 1]; "angle_conf", their product."""
    from . import ops
    if mode not in WEIGHT_MODES[1:]:
        raise ValueError(f"view_weights: mode must be one of {WEIGHT_MODES[1:]}, got {mode!r}")
    if mode != "angle" and conf is None:
        raise ValueError(f"view_weights: mode {mode!r} needs conf, the confidence map of the view")
    if not isinstance(depth, torch.Tensor) or depth.dim() != 2 or depth.dtype != torch.float32:
        raise ValueError(f"view_weights: depth must be a float32 [h,w] tensor, got {getattr(depth, 'dtype', type(depth))} "
                         f"{tuple(getattr(depth, 'shape', ()))}")
    h, w = depth.shape
    if tuple(mask.shape) != (h, w) or tuple(cam.shape) != (2, 4, 4):
        raise ValueError(f"view_weights: for depth {(h, w)} mask must be [h,w] and cam [2,4,4], got {tuple(mask.shape)}, "
                         f"{tuple(cam.shape)}")
    if not depth.is_cuda:
        raise RuntimeError("view_weights: depth must be a ROCm (cuda) tensor; there is no CPU fallback")
    dev = depth.device
    use_conf = mode != "angle"
    if use_conf and (tuple(conf.shape) != (h, w) or not conf.is_floating_point()):
        raise ValueError(f"view_weights: conf must be a floating-point {(h, w)} tensor, got {conf.dtype} {tuple(conf.shape)}")
    for t, name in ((mask, "mask"), (conf if use_conf else None, "conf")):
        if t is not None and t.device != dev:
            raise RuntimeError(f"view_weights: {name} must be on {dev}; there is no CPU fallback")
    cam32 = cam.detach().to("cpu", torch.float32)
    K, E = cam32[1, :3, :3], cam32[0]
    if K[1, 0] != 0 or K[2].tolist() != [0.0, 0.0, 1.0]:
        raise ValueError(f"view_weights: the intrinsic must have the rows (fx, s, cx), (0, fy, cy), (0, 0, 1), got {K.tolist()}")
    depth = depth.contiguous()
    mask = (mask != 0).to(torch.uint8).contiguous()
    normals = ok = None
    if mode != "conf":
        normals, ok = ops.depth_normals(depth, K, E, valid=mask, radius=radius, jump=jump, min_pts=min_pts)
    if use_conf:
        conf = conf.to(torch.float32).contiguous()
    cam_host = torch.cat([K.reshape(9), E.reshape(16)]).contiguous()
    out = torch.empty((h, w), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().cds_tsdf_view_weights(depth.data_ptr(), mask.data_ptr(), normals.data_ptr() if normals is not None else None,
                                                ok.data_ptr() if ok is not None else None, conf.data_ptr() if use_conf else None,
                                                cam_host.data_ptr(), h, w, out.data_ptr(), _stream(dev)), "cds_tsdf_view_weights")
    return out


# -------------------------------------------------------------------------------------------------------------- components
def _check_faces_layout(faces, what: str) -> None:
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{what}: faces must be an int32 [F,3] tensor, got {getattr(faces, 'dtype', type(faces))} "
                         f"{tuple(getattr(faces, 'shape', ()))}")


def _check_index_range(faces: Tensor, nv: int, what: str) -> None:
    if faces.shape[0]:
        lo, hi = (int(x) for x in torch.aminmax(faces))
        if lo < 0 or hi >= nv:
            raise ValueError(f"{what}: faces index outside the {nv} vertices ({lo}..{hi})")


def _check_faces(faces, n_vertices, what: str) -> int:
    """The checks of a face list alone, in the order of a mesh's: layout (ValueError), device (RuntimeError), index range
    (ValueError) -> V."""
    _check_faces_layout(faces, what)
    nv = int(n_vertices)
    if not (0 <= nv < 2 ** 31):
        raise ValueError(f"{what}: {n_vertices} vertices, 0 .. 2^31 - 1 expected")
    if not faces.is_cuda:
        raise RuntimeError(f"{what}: faces must be a ROCm (cuda) tensor; there is no CPU fallback")
    _check_index_range(faces, nv, what)
    return nv


def _labels(faces: Tensor, nv: int):
    """Rules 1-3 of DESIGN §1.11 for a checked, contiguous face list with nv > 0 -> (label int32 [nv], count int32 [nv], rounds)."""
    dev, nf = faces.device, int(faces.shape[0])
    if nf == 0:
        return torch.arange(nv, dtype=torch.int32, device=dev), torch.zeros(nv, dtype=torch.int32, device=dev), 0
    lib = _lib.load()
    parent = torch.empty(nv, dtype=torch.int32, device=dev)
    count = torch.zeros(nv, dtype=torch.int32, device=dev)
    changed = torch.zeros(MAX_ROUNDS, dtype=torch.int32, device=dev)       # one word per round, zeroed once
    with torch.cuda.device(dev):
        stream = _stream(dev)
        check(lib.cds_mesh_cc_init(parent.data_ptr(), nv, stream), "cds_mesh_cc_init")
        rounds = 0
        while True:
            if rounds == MAX_ROUNDS:
                raise RuntimeError(f"mesh_components: the labels of {nv} vertices and {nf} faces did not settle in {MAX_ROUNDS} rounds")
            check(lib.cds_mesh_cc_hook(faces.data_ptr(), nf, nv, parent.data_ptr(), changed.data_ptr() + 4 * rounds, stream),
                  "cds_mesh_cc_hook")
            check(lib.cds_mesh_cc_jump(parent.data_ptr(), nv, stream), "cds_mesh_cc_jump")
            rounds += 1
            if int(changed[rounds - 1]) == 0:                               # the one word read per round
                break
        check(lib.cds_mesh_cc_count(faces.data_ptr(), nf, nv, parent.data_ptr(), count.data_ptr(), stream), "cds_mesh_cc_count")
    return parent, count, rounds


def mesh_components(faces: Tensor, n_vertices: int) -> Dict[str, object]:
    """The connected components of a mesh (DESIGN §1.11 rules 1-3): faces int32 [F,3] on a ROCm device, every index in
    [0, n_vertices) -> {"label" int32 [V]: the smallest vertex of each vertex's component, "components" int32 [C]: the labels,
    ascending, "faces" int64 [C]: the faces of each (a face counts for its first vertex), "rounds": hook passes made}, on that
    device.  Two vertices are connected when a face holds both; a vertex in no face is a component with 0 faces."""
    nv = _check_faces(faces, n_vertices, "mesh_components")
    dev = faces.device
    if nv == 0:
        return {"label": torch.zeros(0, dtype=torch.int32, device=dev), "components": torch.zeros(0, dtype=torch.int32, device=dev),
                "faces": torch.zeros(0, dtype=torch.int64, device=dev), "rounds": 0}
    label, count, rounds = _labels(faces.contiguous(), nv)
    comps = torch.nonzero(label == torch.arange(nv, dtype=torch.int32, device=dev)).reshape(-1)
    return {"label": label, "components": comps.to(torch.int32), "faces": count[comps].to(torch.int64), "rounds": rounds}


def select_components(counts: Tensor, min_faces: int = 0, keep_largest: int = 0) -> Tensor:
    """Rule 4 of DESIGN §1.11: counts [C] in ascending label order -> bool [C].  A component is kept iff count >= min_faces and,
    with K = keep_largest > 0, it is among the first K by (count descending, label ascending) of all components."""
    keep = counts >= int(min_faces)
    if int(keep_largest) > 0:
        order = torch.sort(-counts.to(torch.int64), stable=True).indices   # stable: equal counts stay in label order
        first = torch.zeros_like(keep)
        first[order[:int(keep_largest)]] = True
        keep = keep & first
    return keep


def check_mesh_layout(vert, col, faces, what: str) -> int:
    """The first half of a mesh's checks, the layouts (ValueError): vertices float32 [V,3], colors uint8 [V,3] or None, faces int32
    [F,3] -> V.  render.render_mesh makes its own checks between the two halves."""
    if not isinstance(vert, torch.Tensor) or vert.dim() != 2 or vert.shape[1] != 3 or vert.dtype != torch.float32:
        raise ValueError(f"{what}: vertices must be a float32 [V,3] tensor, got {getattr(vert, 'dtype', type(vert))} "
                         f"{tuple(getattr(vert, 'shape', ()))}")
    nv = int(vert.shape[0])
    if col is not None and (not isinstance(col, torch.Tensor) or tuple(col.shape) != (nv, 3) or col.dtype != torch.uint8):
        raise ValueError(f"{what}: colors must be a uint8 [{nv},3] tensor, got {getattr(col, 'dtype', type(col))} "
                         f"{tuple(getattr(col, 'shape', ()))}")
    _check_faces_layout(faces, what)
    return nv


def check_mesh_device(vert: Tensor, col: Optional[Tensor], faces: Tensor, what: str):
    """The second half: one ROCm device (RuntimeError), then every index of faces inside the vertices (ValueError) -> device."""
    if not vert.is_cuda:
        raise RuntimeError(f"{what}: vertices must be a ROCm (cuda) tensor; there is no CPU fallback")
    dev = vert.device
    for t, name in ((faces, "faces"), (col, "colors")):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{what}: {name} must be on {dev}; there is no CPU fallback")
    _check_index_range(faces, int(vert.shape[0]), what)
    return dev


def _check_mesh(mesh_dict, what: str):
    """The checks of a mesh dict -> (vertices, colors, faces, V, device)."""
    vert, col, faces = mesh_dict["vertices"], mesh_dict["colors"], mesh_dict["faces"]
    nv = check_mesh_layout(vert, col, faces, what)
    return vert, col, faces, nv, check_mesh_device(vert, col, faces, what)


def _kept_rows(vkeep: Tensor, fkeep: Tensor, own):
    """What follows a mark kernel.  vkeep uint8 [V], fkeep uint8 [F]: the keep flags; own: device scalars of the caller's, read
    with the two counts in ONE transfer -> ([kept vertices, kept faces, *own] as ints; None when no vertex is kept, else
    (vertex_new, face_new: the exclusive prefix sums of the flags as int32, the mesh dict to gather into))."""
    vend, fend = torch.cumsum(vkeep, 0, dtype=torch.int64), torch.cumsum(fkeep, 0, dtype=torch.int64)
    n = [int(x) for x in torch.stack([vend[-1], fend[-1], *own]).cpu()]
    if n[0] == 0:
        return n, None
    return n, ((vend - vkeep).to(torch.int32), (fend - fkeep).to(torch.int32), _empty_mesh(vkeep.device, n[0], n[1]))


def clean_mesh(mesh_dict: Dict[str, Tensor], min_faces: int = 0, keep_largest: int = 0):
    """Drop the small connected components of a mesh: ``mesh_dict`` as :meth:`TsdfVolume.extract` returns it
    (vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3], on one ROCm device).  A component is kept iff it has at least
    ``min_faces`` faces and, with ``keep_largest = K > 0``, is one of the K largest (ties: the lower label).  -> (mesh dict of
    the kept faces and the vertices they hold, both in their order, the rows copied bit for bit; info: {"components",
    "vertices", "faces": (before, after), "largest": faces of the largest component, "rounds"}).  "components" counts every
    component before, isolated vertices included, and the kept ones that hold a face after."""
    what = "clean_mesh"
    min_faces, keep_largest = int(min_faces), int(keep_largest)
    if min_faces < 0 or keep_largest < 0:
        raise ValueError(f"{what}: min_faces and keep_largest must be >= 0, got {min_faces} and {keep_largest}")
    vert, col, faces, nv, dev = _check_mesh(mesh_dict, what)
    nf = int(faces.shape[0])
    if nv == 0 or nf == 0:                                                   # no face: no vertex is in a kept face
        return _empty_mesh(dev), {"components": (nv, 0), "vertices": (nv, 0), "faces": (0, 0), "largest": 0, "rounds": 0}
    vert, col, faces = vert.contiguous(), col.contiguous(), faces.contiguous()
    label, count, rounds = _labels(faces, nv)
    comps = torch.nonzero(label == torch.arange(nv, dtype=torch.int32, device=dev)).reshape(-1)
    counts = count[comps]
    kept = select_components(counts, min_faces, keep_largest)
    keep = torch.zeros(nv, dtype=torch.uint8, device=dev)
    keep[comps] = kept.to(torch.uint8)
    fkeep = torch.empty(nf, dtype=torch.uint8, device=dev)
    vkeep = torch.zeros(nv, dtype=torch.uint8, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = _stream(dev)
        check(lib.cds_mesh_cc_mark(faces.data_ptr(), nf, nv, label.data_ptr(), keep.data_ptr(), fkeep.data_ptr(), vkeep.data_ptr(),
                                   stream), "cds_mesh_cc_mark")
        (nv_out, nf_out, n_comp, largest), rows = _kept_rows(vkeep, fkeep, ((kept & (counts > 0)).sum(), counts.max()))
        info = {"components": (int(comps.numel()), n_comp), "vertices": (nv, nv_out), "faces": (nf, nf_out), "largest": largest,
                "rounds": rounds}
        if rows is None:
            return _empty_mesh(dev), info
        vnew, fnew, out = rows
        check(lib.cds_mesh_cc_gather(vert.data_ptr(), col.data_ptr(), faces.data_ptr(), nv, nf, vkeep.data_ptr(), vnew.data_ptr(),
                                     fkeep.data_ptr(), fnew.data_ptr(), nv_out, nf_out, out["vertices"].data_ptr(),
                                     out["colors"].data_ptr(), out["faces"].data_ptr(), stream), "cds_mesh_cc_gather")
    return out, info


# ---------------------------------------------------------------------------------------------------------- simplification
def check_cell(cell, what: str = "simplify_mesh") -> float:
    """-> cell as a float; ValueError unless it is finite and > 0."""
    return _positive(cell, "cell", what)


def _first_of_identity(ident: Tensor, n_clusters: int) -> Tensor:
    """ident int64 [N,3] in ascending face order -> bool [N]: the row is the first with its triple (rule 5's lowest index).
    Stable sorts keep equal triples in face order, so the first of a run is the lowest face: one sort of a packed key while a
    cluster fits PACK_BITS bits, else one per column, last column first."""
    n = int(ident.shape[0])
    if int(n_clusters) <= 1 << PACK_BITS:
        key = (ident[:, 0] << (2 * PACK_BITS)) | (ident[:, 1] << PACK_BITS) | ident[:, 2]
        order = torch.sort(key, stable=True).indices
        key = key[order]
        new = key[1:] != key[:-1]
    else:
        order = torch.sort(ident[:, 2], stable=True).indices
        order = order[torch.sort(ident[order, 1], stable=True).indices]
        order = order[torch.sort(ident[order, 0], stable=True).indices]
        rows = ident[order]
        new = (rows[1:] != rows[:-1]).any(1)
    first = torch.zeros(n, dtype=torch.bool, device=ident.device)
    first[order[:1]] = True
    first[order[1:][new]] = True
    return first


def _clusters(vert: Tensor, col: Tensor, faces: Tensor, cell: float, placement: str):
    """Rules 1-4 and the face pass of rule 5 for checked, contiguous tensors with V > 0 and F > 0, on the current device
    -> (C, positions float32 [C,3], packed colours int32 [C], fallback uint8 [C] or None for "mean", face clusters int32 [F,3],
    collapsed uint8 [F], identities int32 [F,3])."""
    from .pointcloud import pack_colors, voxel_groups
    dev, nv, nf = vert.device, int(vert.shape[0]), int(faces.shape[0])
    lib = _lib.load()
    stream = _stream(dev)
    perm, start, ukeys, counts = voxel_groups(vert, cell, "simplify_mesh")   # ValueError for a vertex that is not finite
    nc = int(ukeys.numel())
    cluster = torch.empty(nv, dtype=torch.int32, device=dev)
    cluster[perm] = torch.repeat_interleave(torch.arange(nc, dtype=torch.int32, device=dev), counts, output_size=nv)
    mean = torch.empty((nc, 3), dtype=torch.float32, device=dev)
    packed = torch.empty(nc, dtype=torch.int32, device=dev)
    members = torch.empty(nc, dtype=torch.int32, device=dev)
    check(lib.cds_voxel_merge_f32(vert.data_ptr(), pack_colors(col).data_ptr(), None, nv, perm.data_ptr(), start.data_ptr(), nc,
                                  mean.data_ptr(), packed.data_ptr(), None, members.data_ptr(), stream), "cds_voxel_merge_f32")
    fclus = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    ident = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    gone = torch.empty(nf, dtype=torch.uint8, device=dev)
    check(lib.cds_mesh_simplify_faces(faces.data_ptr(), nf, nv, cluster.data_ptr(), nc, fclus.data_ptr(), gone.data_ptr(),
                                      ident.data_ptr(), stream), "cds_mesh_simplify_faces")
    if placement != "quadric":
        return nc, mean, packed, None, fclus, gone, ident
    owner, inc = torch.sort(fclus.reshape(-1), stable=True)                  # the corners 3 f + j of every cluster, ascending
    inc_start = torch.searchsorted(owner, torch.arange(nc + 1, dtype=torch.int32, device=dev)).to(torch.int32)
    pos = torch.empty((nc, 3), dtype=torch.float32, device=dev)
    fell = torch.empty(nc, dtype=torch.uint8, device=dev)
    check(lib.cds_mesh_simplify_quadric_f32(vert.data_ptr(), nv, faces.data_ptr(), nf, perm.data_ptr(), start.data_ptr(),
                                            inc.data_ptr(), inc_start.data_ptr(), nc, cell, pos.data_ptr(), fell.data_ptr(),
                                            stream), "cds_mesh_simplify_quadric_f32")
    return nc, pos, packed, fell, fclus, gone, ident


def simplify_mesh(mesh_dict: Dict[str, Tensor], cell: float, placement: str = "quadric"):
    """Vertex clustering with quadric placement: ``mesh_dict`` as :meth:`TsdfVolume.extract` returns it (vertices
    float32 [V,3], all finite, colors uint8 [V,3], faces int32 [F,3], on one ROCm device).  The vertices of a cell of side ``cell``
    (world units; the cells of ``--merge_voxel``: :func:`pointcloud.voxel_groups`) become one vertex: at the regularised minimiser
    of its faces' quadric error (``placement="quadric"``; it falls back to the mean where that is undetermined or leaves the
    neighbourhood) or at their mean (``"mean"``, the bits of ``cds_voxel_merge_f32``), with the rounded mean colour.  Faces with two
    corners in one cluster and repeats of an earlier face are dropped, as are clusters no surviving face holds.  -> (mesh dict: the
    surviving faces in their order, the clusters they hold in ascending cell-key order; info: {"vertices", "faces": (before,
    after), "clusters", "collapsed", "duplicates", "fallback": clusters, kept or not, that fell back (0 for "mean")})."""
    what = "simplify_mesh"
    cell = check_cell(cell, what)
    if placement not in PLACEMENTS:
        raise ValueError(f"{what}: placement must be one of {PLACEMENTS}, got {placement!r}")
    vert, col, faces, nv, dev = _check_mesh(mesh_dict, what)
    nf = int(faces.shape[0])
    if nv == 0 or nf == 0:                                                   # no face: no cluster is in a surviving face
        return _empty_mesh(dev), {"vertices": (nv, 0), "faces": (0, 0), "clusters": 0, "collapsed": 0, "duplicates": 0, "fallback": 0}
    if 3 * nf >= 2 ** 31:
        raise ValueError(f"{what}: {nf} faces, at most {(2 ** 31 - 1) // 3}")
    vert, col, faces = vert.contiguous(), col.contiguous(), faces.contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = _stream(dev)
        nc, pos, packed, fell, fclus, gone, ident = _clusters(vert, col, faces, cell, placement)
        n_fell = fell.sum() if fell is not None else torch.zeros((), dtype=torch.int64, device=dev)
        alive = torch.nonzero(gone == 0).reshape(-1)
        fkeep = torch.zeros(nf, dtype=torch.uint8, device=dev)
        if alive.numel():
            fkeep[alive[_first_of_identity(ident[alive].long(), nc)]] = 1
        ckeep = torch.zeros(nc, dtype=torch.uint8, device=dev)
        check(lib.cds_mesh_simplify_mark(fclus.data_ptr(), fkeep.data_ptr(), nf, nc, ckeep.data_ptr(), stream),
              "cds_mesh_simplify_mark")
        (nv_out, nf_out, n_gone, n_fell), rows = _kept_rows(ckeep, fkeep, (gone.sum(), n_fell))
        info = {"vertices": (nv, nv_out), "faces": (nf, nf_out), "clusters": nc, "collapsed": n_gone,
                "duplicates": nf - n_gone - nf_out, "fallback": n_fell}
        if rows is None:
            return _empty_mesh(dev), info
        cnew, fnew, out = rows
        check(lib.cds_mesh_simplify_gather(pos.data_ptr(), packed.data_ptr(), nc, ckeep.data_ptr(), cnew.data_ptr(), fclus.data_ptr(),
                                           nf, fkeep.data_ptr(), fnew.data_ptr(), nv_out, nf_out, out["vertices"].data_ptr(),
                                           out["colors"].data_ptr(), out["faces"].data_ptr(), stream), "cds_mesh_simplify_gather")
    return out, info


# --------------------------------------------------------------------------------------------------------------- smoothing
def check_smooth(iterations, lam=0.5, mu=-0.53, max_move=0.0, what: str = "smooth_mesh"):
    """-> (iterations, lam, mu, max_move) as an int and three floats; ValueError unless iterations is an int in 1..MAX_SMOOTH,
    lam is finite and in (0, 1], mu is finite and in [-1, 0] and max_move is finite and >= 0 (rule 7 of DESIGN §1.15)."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not (1 <= int(iterations) <= MAX_SMOOTH):
        raise ValueError(f"{what}: iterations must be an int in 1..{MAX_SMOOTH}, got {iterations!r}")
    values = []
    for value, name, ok, span in ((lam, "lam", lambda x: 0.0 < x <= 1.0, "(0, 1]"), (mu, "mu", lambda x: -1.0 <= x <= 0.0, "[-1, 0]"),
                                  (max_move, "max_move", lambda x: x >= 0.0, "[0, inf)")):
        try:
            x = float(value)
        except (TypeError, ValueError):
            x = math.nan
        if not (math.isfinite(x) and ok(x)):
            raise ValueError(f"{what}: {name} must be finite and in {span}, got {value!r}")
        values.append(x)
    return (int(iterations), *values)


def _adjacency(faces: Tensor, nv: int):
    """Rules 1-3 of DESIGN §1.15 for a contiguous int32 [F,3] face list on the current device, nv > 0 -> None when no valid edge
    slot exists, else (start int32 [nv+1], deg int32 [nv], nbr int32 [E], flags uint8 [nv]).  The counting build: a count pass, the
    prefix sum, a fill pass at integer cursors and the finishing kernel; the segments longer than ADJ_SMALL, which that kernel
    does not sort itself, go through one torch sort of just their entries."""
    dev, nf = faces.device, int(faces.shape[0])
    if nf == 0:
        return None
    if 6 * nf >= 2 ** 31:
        raise ValueError(f"mesh_adjacency: {nf} faces, at most {(2 ** 31 - 1) // 6}")
    lib, stream = _lib.load(), _stream(dev)
    count = torch.zeros(nv, dtype=torch.int32, device=dev)
    check(lib.cds_mesh_adj_count(faces.data_ptr(), nf, nv, count.data_ptr(), stream), "cds_mesh_adj_count")
    start = torch.zeros(nv + 1, dtype=torch.int32, device=dev)
    start[1:] = torch.cumsum(count, 0, dtype=torch.int32)
    long_ones = torch.nonzero(count > ADJ_SMALL).reshape(-1)
    ne = int(start[-1])                                                      # the one read of the build, after nonzero's
    if ne == 0:
        return None
    nbr = torch.empty(ne, dtype=torch.int32, device=dev)
    cursor = torch.zeros(nv, dtype=torch.int32, device=dev)
    check(lib.cds_mesh_adj_fill(faces.data_ptr(), nf, nv, start.data_ptr(), cursor.data_ptr(), nbr.data_ptr(), ne, stream),
          "cds_mesh_adj_fill")
    if long_ones.numel():
        lens = count[long_ones].long()
        owner = torch.repeat_interleave(torch.arange(long_ones.numel(), device=dev), lens)
        first = torch.cumsum(lens, 0) - lens
        at = start[long_ones].long()[owner] + (torch.arange(owner.numel(), device=dev) - first[owner])
        nbr[at] = (torch.sort((owner << 32) | nbr[at].long()).values & 0xffffffff).to(torch.int32)
    deg = torch.empty(nv, dtype=torch.int32, device=dev)
    flags = torch.empty(nv, dtype=torch.uint8, device=dev)
    check(lib.cds_mesh_adj_finish(nv, start.data_ptr(), nbr.data_ptr(), ne, deg.data_ptr(), flags.data_ptr(), stream),
          "cds_mesh_adj_finish")
    return start, deg, nbr, flags


def mesh_adjacency(faces: Tensor, n_vertices: int) -> Dict[str, Tensor]:
    """The neighbours that :func:`smooth_mesh` averages over (DESIGN §1.15 rules 1-3): faces int32 [F,3] on a ROCm device, every
    index in [0, n_vertices) -> the CSR the step kernel reads, on that device: {"start" int32 [V+1]: vertex v owns
    ``neighbors[start[v] : start[v+1]]``, of which the first ``degree[v]`` are its neighbours, ascending (the rest is slack),
    "degree" int32 [V], "neighbors" int32 [E], "boundary" bool [V]: the vertex has an edge that one face slot holds, and its
    neighbours are then only those across such edges, "isolated" bool [V]: no neighbour}."""
    nv = _check_faces(faces, n_vertices, "mesh_adjacency")
    dev = faces.device
    with torch.cuda.device(dev):
        built = _adjacency(faces.contiguous(), nv) if nv else None
    if built is None:
        return {"start": torch.zeros(nv + 1, dtype=torch.int32, device=dev), "degree": torch.zeros(nv, dtype=torch.int32, device=dev),
                "neighbors": torch.zeros(0, dtype=torch.int32, device=dev), "boundary": torch.zeros(nv, dtype=torch.bool, device=dev),
                "isolated": torch.ones(nv, dtype=torch.bool, device=dev)}
    start, deg, nbr, flags = built
    return {"start": start, "degree": deg, "neighbors": nbr, "boundary": (flags & ADJ_BOUNDARY) != 0,
            "isolated": (flags & ADJ_ISOLATED) != 0}


def smooth_mesh(mesh_dict: Dict[str, Tensor], iterations: int, lam: float = 0.5, mu: float = -0.53, max_move: float = 0.0):
    """Taubin's lambda|mu filter with uniform weights: ``mesh_dict`` as :meth:`TsdfVolume.extract` returns it
    (vertices float32 [V,3], all finite, colors uint8 [V,3], faces int32 [F,3], on one ROCm device).  ``iterations`` times, every
    vertex moves by ``lam`` towards the mean of its neighbours and then, unless ``mu`` is 0 (the plain Laplacian filter, which
    shrinks), by ``mu`` < 0 away from the new one; a vertex on an open border averages over its border neighbours only, and one
    without neighbours stays.  ``max_move`` > 0 (world units) then pulls every vertex back to within that distance of where it
    was.  Only the positions change: colours and faces are the input's tensors.  -> (mesh dict; info: {"iterations", "lam", "mu",
    "vertices": V, "boundary", "isolated", "clamped": vertices, "max_move": the largest move, before the limit})."""
    what = "smooth_mesh"
    iterations, lam, mu, max_move = check_smooth(iterations, lam, mu, max_move, what)
    vert, col, faces, nv, dev = _check_mesh(mesh_dict, what)
    if nv and not bool(torch.isfinite(vert).all()):
        raise ValueError(f"{what}: vertices must be finite")
    info = {"iterations": iterations, "lam": lam, "mu": mu, "vertices": nv, "boundary": 0, "isolated": nv, "clamped": 0,
            "max_move": 0.0}
    same = {"vertices": vert, "colors": col, "faces": faces}
    if nv == 0:
        return same, info
    vert, faces = vert.contiguous(), faces.contiguous()
    with torch.cuda.device(dev):
        built = _adjacency(faces, nv)
        if built is None:                                                    # no valid edge: every vertex is isolated
            return same, info
        start, deg, nbr, flags = built
        lib, stream = _lib.load(), _stream(dev)
        src, dst = vert, torch.empty_like(vert)
        spare = None
        for _ in range(iterations):
            for factor in (lam, mu):
                if factor == 0.0:
                    continue
                check(lib.cds_mesh_smooth_step_f32(src.data_ptr(), dst.data_ptr(), nv, start.data_ptr(), deg.data_ptr(),
                                                   nbr.data_ptr(), factor, stream), "cds_mesh_smooth_step_f32")
                if src is vert:                                              # the input is read, never written
                    spare = torch.empty_like(vert)
                    src, dst = dst, spare
                else:
                    src, dst = dst, src
        move2 = torch.empty(nv, dtype=torch.float64, device=dev)
        clamped = torch.empty(nv, dtype=torch.uint8, device=dev)
        check(lib.cds_mesh_smooth_limit_f32(vert.data_ptr(), src.data_ptr(), nv, max_move, move2.data_ptr(), clamped.data_ptr(),
                                            stream), "cds_mesh_smooth_limit_f32")
        stats = torch.stack([move2.max(), ((flags & ADJ_BOUNDARY) != 0).sum().double(), ((flags & ADJ_ISOLATED) != 0).sum().double(),
                             clamped.sum().double()]).cpu().tolist()           # the one read after the launches
    info.update(boundary=int(stats[1]), isolated=int(stats[2]), clamped=int(stats[3]), max_move=math.sqrt(stats[0]))
    return {"vertices": src, "colors": col, "faces": faces}, info


# ------------------------------------------------------------------------------------------------------------ hole filling
def check_fill(max_edges, what: str = "fill_holes") -> int:
    """-> max_edges as an int; ValueError unless it is an int in 3..MAX_FILL_EDGES.  The upper end is there because one thread
    walks a loop from end to end (rule 4 of DESIGN §1.20)."""
    if isinstance(max_edges, bool) or not isinstance(max_edges, (int, np.integer)) or not (3 <= int(max_edges) <= MAX_FILL_EDGES):
        raise ValueError(f"{what}: max_edges must be an int in 3..{MAX_FILL_EDGES} (one thread walks a hole's rim), got {max_edges!r}")
    return int(max_edges)


def _borders(faces: Tensor, nv: int, what: str):
    """Rules 1-3 of DESIGN §1.20 for a contiguous int32 [F,3] face list on the current device, nv > 0 and F > 0 -> (next int32
    [nv], -1 where the vertex is not regular, regular uint8 [nv], the border half-edges that leave each vertex int32 [nv], and the
    two pairs (label, jump) int32 [2,nv] at the start of the pointer doubling, along next and along prev).  One key per half-edge,
    one torch sort of the keys, the border kernel over the sorted keys and the kernel of rule 3."""
    dev, nf = faces.device, int(faces.shape[0])
    if 3 * nf >= 2 ** 31:
        raise ValueError(f"{what}: {nf} faces, at most {(2 ** 31 - 1) // 3}")
    lib, stream = _lib.load(), _stream(dev)
    keys = torch.empty(3 * nf, dtype=torch.int64, device=dev)
    check(lib.cds_mesh_fill_keys(faces.data_ptr(), nf, nv, keys.data_ptr(), stream), "cds_mesh_fill_keys")
    keys = torch.sort(keys).values
    leave = torch.zeros(nv, dtype=torch.int32, device=dev)
    enter = torch.zeros(nv, dtype=torch.int32, device=dev)
    nxt = torch.full((nv,), -1, dtype=torch.int32, device=dev)
    prv = torch.full((nv,), -1, dtype=torch.int32, device=dev)
    check(lib.cds_mesh_fill_borders(keys.data_ptr(), 3 * nf, nv, leave.data_ptr(), enter.data_ptr(), nxt.data_ptr(), prv.data_ptr(),
                                    stream), "cds_mesh_fill_borders")
    regular = torch.empty(nv, dtype=torch.uint8, device=dev)
    pairs = [torch.empty((2, nv), dtype=torch.int32, device=dev) for _ in range(4)]
    check(lib.cds_mesh_fill_init(nv, leave.data_ptr(), enter.data_ptr(), nxt.data_ptr(), prv.data_ptr(), regular.data_ptr(),
                                 *(t.data_ptr() for t in pairs), stream), "cds_mesh_fill_init")
    return nxt, regular, leave, pairs


def mesh_borders(faces: Tensor, n_vertices: int) -> Dict[str, object]:
    """The border loops that :func:`fill_holes` walks (DESIGN §1.20 rules 1-3): faces int32 [F,3] on a ROCm device, every index in
    [0, n_vertices) -> {"next" int32 [V]: the end of the one border half-edge that leaves a regular vertex, -1 where the vertex is
    not regular, "regular" bool [V]: exactly one border half-edge leaves the vertex and exactly one enters it, "border_edges":
    the half-edges whose edge one face slot holds, an int}, on that device."""
    nv = _check_faces(faces, n_vertices, "mesh_borders")
    dev = faces.device
    if nv == 0 or faces.shape[0] == 0:
        return {"next": torch.full((nv,), -1, dtype=torch.int32, device=dev), "regular": torch.zeros(nv, dtype=torch.bool, device=dev),
                "border_edges": 0}
    with torch.cuda.device(dev):
        nxt, regular, leave, _ = _borders(faces.contiguous(), nv, "mesh_borders")
        return {"next": nxt, "regular": regular != 0, "border_edges": int(leave.sum())}


def fill_holes(mesh_dict: Dict[str, Tensor], max_edges: int):
    """Close the small holes of a mesh with centroid fans: ``mesh_dict`` as :meth:`TsdfVolume.extract` returns it
    (vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3], on one ROCm device).  A border edge is one that a single face
    slot holds; a hole is a cycle of border edges through vertices that each have one border edge coming and one going.  A hole of
    3 .. ``max_edges`` edges is filled: one of 3 with one face, a larger one with a new vertex at the mean of its rim (position
    summed in fp64 in loop order, colour rounded in integers) and one face per border edge, each running its edge backwards and
    so oriented as the surface around it.  Larger loops (the outer rim of an open scan), holes that touch in a vertex and
    non-manifold edges stay as they are.  The fan is flat: :func:`smooth_mesh` after it fairs the cap.  -> (mesh dict: the input's
    rows bit for bit, then the new vertices and the new faces in ascending order of each loop's smallest vertex; info:
    {"max_edges", "loops": filled, "largest": edges of the largest filled loop, "border_edges", "vertices", "faces": (before,
    after)}).  A mesh in which nothing is filled comes back as the input's own tensors.  There is no CPU fallback."""
    what = "fill_holes"
    max_edges = check_fill(max_edges, what)
    vert, col, faces, nv, dev = _check_mesh(mesh_dict, what)
    nf = int(faces.shape[0])
    same = {"vertices": vert, "colors": col, "faces": faces}
    info = {"max_edges": max_edges, "loops": 0, "largest": 0, "border_edges": (0, 0), "vertices": (nv, nv), "faces": (nf, nf)}
    if nv == 0 or nf == 0:
        return same, info
    vert, col, faces = vert.contiguous(), col.contiguous(), faces.contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = _stream(dev)
        nxt, regular, leave, (label, jump, label_b, jump_b) = _borders(faces, nv, what)
        n_border = int(leave.sum())                                          # the read that ends the detection
        info["border_edges"] = (n_border, n_border)
        if n_border == 0:
            return same, info
        ring = torch.nonzero(regular).reshape(-1).to(torch.int32)             # the regular vertices, ascending
        m = int(ring.numel())
        if m == 0:
            return same, info
        for _ in range((max_edges - 1).bit_length()):                        # windows of 2^rounds >= max_edges vertices
            check(lib.cds_mesh_fill_double(ring.data_ptr(), m, nv, label.data_ptr(), jump.data_ptr(), label_b.data_ptr(),
                                           jump_b.data_ptr(), stream), "cds_mesh_fill_double")
            label, jump, label_b, jump_b = label_b, jump_b, label, jump
        edges = torch.empty(m, dtype=torch.int32, device=dev)
        centre = torch.empty((m, 3), dtype=torch.float32, device=dev)
        centre_color = torch.empty((m, 3), dtype=torch.uint8, device=dev)
        check(lib.cds_mesh_fill_walk(vert.data_ptr(), col.data_ptr(), nv, nxt.data_ptr(), regular.data_ptr(), label.data_ptr(),
                                     ring.data_ptr(), m, max_edges, edges.data_ptr(), centre.data_ptr(), centre_color.data_ptr(),
                                     stream), "cds_mesh_fill_walk")
        fan = (edges >= 4).to(torch.int64)
        made = torch.where(edges == 3, 1, edges).to(torch.int64)
        vend, fend = torch.cumsum(fan, 0), torch.cumsum(made, 0)
        loops, new_v, new_f, largest, closed = (int(x) for x in torch.stack(
            [(edges > 0).sum(), vend[-1], fend[-1], edges.max().long(), edges.sum()]).cpu())          # the ONE read of the fill
        info.update(loops=loops, largest=largest, border_edges=(n_border, n_border - closed), vertices=(nv, nv + new_v),
                    faces=(nf, nf + new_f))
        if loops == 0:
            return same, info
        if nv + new_v >= 2 ** 31 or nf + new_f >= 2 ** 31:
            raise ValueError(f"{what}: {nv + new_v} vertices and {nf + new_f} faces after the fill, at most 2^31 - 1 each")
        out = _empty_mesh(dev, nv + new_v, nf + new_f)
        out["vertices"][:nv].copy_(vert)
        out["colors"][:nv].copy_(col)
        out["faces"][:nf].copy_(faces)
        vertex_at, face_at = vend - fan, fend - made                         # the exclusive prefix sums
        check(lib.cds_mesh_fill_emit(nxt.data_ptr(), regular.data_ptr(), nv, nf, ring.data_ptr(), m, max_edges, edges.data_ptr(),
                                     vertex_at.data_ptr(), face_at.data_ptr(), centre.data_ptr(), centre_color.data_ptr(),
                                     new_v, new_f, out["vertices"].data_ptr(), out["colors"].data_ptr(), out["faces"].data_ptr(),
                                     stream), "cds_mesh_fill_emit")
    return out, info


# ---------------------------------------------------------------------------------------------------------------- sampling
def check_spacing(spacing, what: str = "sample_mesh") -> float:
    """-> spacing as a float; ValueError unless it is finite and > 0."""
    return _positive(spacing, "spacing", what)


def sample_mesh(mesh_dict: Dict[str, Tensor], spacing: float, max_points: int = MAX_SAMPLES):
    """A dense, deterministic point set from the faces of a mesh: ``mesh_dict`` as :meth:`TsdfVolume.extract`
    returns it (vertices float32 [V,3], colors uint8 [V,3], faces int32 [F,3], on one ROCm device).  Every face is cut into n^2
    congruent sub-triangles, n the smallest count for which the face's longest edge is at most n ``spacing`` (world units), and
    the centroid of each becomes a point with the interpolated colour: every point of the surface lies within 2/3 ``spacing`` of
    a sample of its face, and no sample lies on an edge.  A face with a corner that is not finite gives nothing.  -> ({"points"
    float32 [N,3], "colors" uint8 [N,3], "face" int32 [N]: the face of each sample}, in face order; info: {"faces", "points",
    "max_n": the largest n, "skipped": faces that gave nothing}).  ValueError, before the samples are allocated, for a face that
    needs n > 2^15 and for more than ``max_points`` samples."""
    what = "sample_mesh"
    spacing = check_spacing(spacing, what)
    vert, col, faces, nv, dev = _check_mesh(mesh_dict, what)
    nf = int(faces.shape[0])
    empty = {"points": torch.zeros((0, 3), dtype=torch.float32, device=dev), "colors": torch.zeros((0, 3), dtype=torch.uint8, device=dev),
             "face": torch.zeros(0, dtype=torch.int32, device=dev)}
    if nf == 0:
        return empty, {"faces": 0, "points": 0, "max_n": 0, "skipped": 0}
    vert, col, faces = vert.contiguous(), col.contiguous(), faces.contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = _stream(dev)
        n = torch.empty(nf, dtype=torch.int32, device=dev)
        n2 = torch.empty(nf, dtype=torch.int64, device=dev)
        check(lib.cds_mesh_sample_count(vert.data_ptr(), nv, faces.data_ptr(), nf, spacing, n.data_ptr(), n2.data_ptr(), stream),
              "cds_mesh_sample_count")
        ends = torch.cumsum(n2, 0)
        total, max_n, skipped = (int(x) for x in torch.stack([ends[-1], n.max().long(), (n == 0).sum()]).cpu())   # the one read
        if max_n > MAX_SAMPLE_N:
            raise ValueError(f"{what}: a face needs more than {MAX_SAMPLE_N} subdivisions at a spacing of {spacing}: raise the "
                             "spacing")
        if total > int(max_points) or total >= 2 ** 31:
            raise ValueError(f"{what}: a spacing of {spacing} gives {total} points, at most {min(int(max_points), 2 ** 31 - 1)}: "
                             "raise the spacing or simplify the mesh first")
        info = {"faces": nf, "points": total, "max_n": max_n, "skipped": skipped}
        if total == 0:
            return empty, info
        offsets = ends - n2
        out = {"points": torch.empty((total, 3), dtype=torch.float32, device=dev),
               "colors": torch.empty((total, 3), dtype=torch.uint8, device=dev),
               "face": torch.empty(total, dtype=torch.int32, device=dev)}
        check(lib.cds_mesh_sample_emit(vert.data_ptr(), col.data_ptr(), nv, faces.data_ptr(), nf, n.data_ptr(), offsets.data_ptr(),
                                       total, out["points"].data_ptr(), out["colors"].data_ptr(), out["face"].data_ptr(), stream),
              "cds_mesh_sample_emit")
    return out, info


def load_mesh(mesh, device="cuda") -> Dict[str, Tensor]:
    """A mesh file of :func:`write_mesh_ply`, or a mesh dict of this module already on the device -> {"vertices", "colors",
    "faces"} on the device."""
    keys = ("vertices", "colors", "faces")
    if isinstance(mesh, dict):
        return {k: mesh[k] for k in keys}
    dev = torch.device(device)
    return {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in zip(keys, read_mesh_ply(str(mesh)))}


def sample_file(path: str, spacing: float, device="cuda", max_points: int = MAX_SAMPLES):
    """The faces of a mesh file of :func:`write_mesh_ply` through :func:`sample_mesh` -> (its result, its info).  ValueError
    that names the file when it holds no face (a cloud: there is no surface to sample)."""
    spacing = check_spacing(spacing, "sample_file")
    try:
        mesh = load_mesh(path, device)
    except ValueError as e:
        raise ValueError(f"{path}: the faces of a mesh are needed to sample its surface, and this is not a mesh file of "
                         f"write_mesh_ply ({e})") from None
    if len(mesh["faces"]) == 0:
        raise ValueError(f"{path}: no faces: there is no surface to sample")
    return sample_mesh(mesh, spacing, max_points)


def write_surface_ply(path: str, mesh_dict: Dict[str, Tensor], spacing: float) -> Dict[str, object]:
    """The sampled surface of a mesh on the device as an ``x y z red green blue`` cloud (:func:`fusion.write_ply`)
    -> sample_mesh's info."""
    out, info = sample_mesh(mesh_dict, spacing)
    write_ply(path, out["points"].cpu().numpy(), out["colors"].cpu().numpy())
    return info


# -------------------------------------------------------------------------------------------------------------------- scans
def _check_weighting(weight, interp, interp_jump, what: str) -> float:
    """-> interp_jump as a float; ValueError for an unknown weight mode or, with interp, a jump that is not finite and > 0."""
    if weight not in WEIGHT_MODES:
        raise ValueError(f"{what}: weight must be one of {WEIGHT_MODES}, got {weight!r}")
    return _positive(interp_jump, "interp_jump", what) if interp else float(interp_jump)


def mesh_views(views: Sequence[dict], voxel: float, trunc: Optional[float] = None, min_weight: int = 2, device="cuda",
               weight: str = "one", interp: bool = False, interp_jump: float = 0.05):
    """Allocation, integration and extraction for the per-view records that ``filter_depth(collect=...)`` gathers
    -> (mesh dict of :meth:`TsdfVolume.extract`, the volume).  ``weight``: "one", or a mode of :func:`view_weights`, whose maps
    (from each record's depth, mask, cam and, for the conf modes, "conf") then weigh the pixels; ``interp`` / ``interp_jump`` as in
    :meth:`TsdfVolume.integrate`.  At their defaults nothing of that runs."""
    interp_jump = _check_weighting(weight, interp, interp_jump, "mesh_views")
    dev = torch.device(device)
    pts = torch.cat([v["points"] for v in views]) if views else torch.zeros((0, 3), dtype=torch.float32, device=dev)
    vol = TsdfVolume(pts, voxel, trunc)
    if views and vol.n_blocks:
        weights = None
        if weight != "one":
            weights = torch.stack([view_weights(v["depth"], v["mask"], v["cam"], v.get("conf"), mode=weight) for v in views])
        vol.integrate(torch.stack([v["depth"] for v in views]), torch.stack([v["mask"] for v in views]),
                      torch.stack([v["image"] for v in views]), torch.stack([v["cam"] for v in views]), weights=weights,
                      interp=bool(interp), interp_jump=interp_jump)
    return vol.extract(min_weight), vol


def _check_sample(sample, surface_ply, what: str) -> float:
    """-> sample as a float, 0.0 for "off"; ValueError for a negative or non-finite spacing or one without a file to write."""
    if sample is None or sample == 0:
        return 0.0
    if surface_ply is None:
        raise ValueError(f"{what}: sample needs surface_ply, the file of the sampled surface")
    return check_spacing(sample, what)


def _check_simplify(simplify, placement, what: str) -> float:
    """-> simplify as a float, 0.0 for "off"; ValueError for a negative or non-finite cell or an unknown placement."""
    if placement not in PLACEMENTS:
        raise ValueError(f"{what}: placement must be one of {PLACEMENTS}, got {placement!r}")
    if simplify is None or simplify == 0:
        return 0.0
    return check_cell(simplify, what)


def _check_fill(fill_holes, what: str) -> int:
    """-> 0 for "off" (fill_holes None or 0), else max_edges through :func:`check_fill` (ValueError)."""
    if fill_holes is None or (not isinstance(fill_holes, bool) and isinstance(fill_holes, (int, np.integer)) and int(fill_holes) == 0):
        return 0
    return check_fill(fill_holes, what)


def _check_smooth(smooth, lam, mu, max_move, what: str):
    """-> None for "off" (smooth None or 0), else (iterations, lam, mu, max_move) through :func:`check_smooth` (ValueError)."""
    if smooth is None or (not isinstance(smooth, bool) and isinstance(smooth, (int, np.integer)) and int(smooth) == 0):
        return None
    return check_smooth(smooth, lam, mu, max_move, what)


def _finish(mesh, plyfilename: str, clean, smooth, simplify: float, placement: str, sample: float, surface_ply,
            fill: int = 0) -> Dict[str, object]:
    """The way of an extracted or loaded mesh into its files: :func:`clean_mesh` with ``clean`` = (min_component, keep_largest)
    unless it is None, :func:`fill_holes` with ``fill`` = max_edges when it is > 0, :func:`smooth_mesh` with ``smooth`` =
    (iterations, lam, mu, max_move) unless it is None,
    :func:`simplify_mesh` when ``simplify`` > 0, the mesh PLY, and when ``sample`` > 0 the sampled surface at ``surface_ply``
    -> {"vertices", "faces", "mesh": the mesh written, on the device[, "clean"][, "fill"][, "smooth"][, "simplify"][, "sample"]}."""
    out = {}
    if clean is not None:
        mesh, out["clean"] = clean_mesh(mesh, *clean)
    if fill > 0:
        mesh, out["fill"] = fill_holes(mesh, fill)
    if smooth is not None:
        mesh, out["smooth"] = smooth_mesh(mesh, *smooth)
        out["smooth"] = dict(out["smooth"], limit=smooth[3])
    if simplify > 0:
        mesh, out["simplify"] = simplify_mesh(mesh, simplify, placement)
    write_mesh_ply(plyfilename, mesh["vertices"].cpu().numpy(), mesh["colors"].cpu().numpy(), mesh["faces"].cpu().numpy())
    if sample > 0:
        out["sample"] = dict(write_surface_ply(surface_ply, mesh, sample), spacing=sample)
    return dict(out, vertices=int(mesh["vertices"].shape[0]), faces=int(mesh["faces"].shape[0]), mesh=mesh)


def mesh_scan(pair_folder: str, scan_folder: str, plyfilename: str, voxel: float, trunc: Optional[float] = None, min_weight: int = 2,
              method: str = "normal", cloud_ply: Optional[str] = None, device: str = "cuda", min_component: int = 0,
              keep_largest: int = 0, simplify: float = 0.0, placement: str = "quadric", sample: float = 0.0,
              surface_ply: Optional[str] = None, weight: str = "one", interp: bool = False, interp_jump: float = 0.05,
              smooth: int = 0, smooth_lambda: float = 0.5, smooth_mu: float = -0.53, smooth_max_move: float = 0.0,
              fill_holes: int = 0, **fusion_options) -> Dict[str, object]:
    """One scan from saved depth maps to a mesh at ``plyfilename``: the fusion pass of :func:`fusion.filter_depth` (``method``
    "normal" or "dynamic" and its ``fusion_options``), then allocation from every view's kept points, integration of the fused
    depth maps in ``pair.txt`` order and extraction.  ``cloud_ply``: also write the fused cloud there, from the same pass and byte
    for byte what ``filter_depth`` writes alone.  ``min_component`` / ``keep_largest``: when either is > 0 the mesh goes through
    :func:`clean_mesh` before it is written; at 0 nothing of that runs.  ``simplify``: a cell side > 0 sends the
    mesh, after the clean-up, through :func:`simplify_mesh` with ``placement``; at 0 nothing of that runs.
    ``sample``: a spacing > 0 also writes the sampled surface of the mesh written (:func:`sample_mesh`) as a cloud
    at ``surface_ply``; at 0 nothing of that runs.  ``weight`` / ``interp`` / ``interp_jump``: the weighted, interpolating
    integration of :func:`mesh_views`; the confidence of the conf modes is the view's last-stage confidence map.
    ``smooth``: iterations > 0 send the mesh, after the clean-up and before the simplification, through :func:`smooth_mesh` with
    ``smooth_lambda``, ``smooth_mu`` and ``smooth_max_move``; at 0 nothing of that runs.  ``fill_holes``: N > 0 sends
    the mesh, after the clean-up and before the smoothing, through :func:`fill_holes` with ``max_edges`` N; at 0
    nothing of that runs.
    -> {"vertices", "faces", "blocks": counts, "cloud": filter_depth's result, "mesh": the mesh dict written, still on the device
    (render.render_scan takes it)[, "clean": clean_mesh's info][, "fill": fill_holes' info][, "smooth": smooth_mesh's info][, "simplify": simplify_mesh's info][, "sample": sample_mesh's
    info and the spacing]}."""
    from .fusion import filter_depth
    if method == "gipuma":
        raise ValueError("mesh_scan: gipuma fusion is not supported (its fused point has no single depth map); use normal or dynamic")
    voxel, trunc = check_voxel(voxel, trunc, "mesh_scan")
    if int(min_weight) < 1:
        raise ValueError(f"mesh_scan: min_weight must be >= 1, got {min_weight}")
    if int(min_component) < 0 or int(keep_largest) < 0:
        raise ValueError(f"mesh_scan: min_component and keep_largest must be >= 0, got {min_component} and {keep_largest}")
    simplify = _check_simplify(simplify, placement, "mesh_scan")
    sample = _check_sample(sample, surface_ply, "mesh_scan")
    smooth = _check_smooth(smooth, smooth_lambda, smooth_mu, smooth_max_move, "mesh_scan")
    fill = _check_fill(fill_holes, "mesh_scan")
    interp_jump = _check_weighting(weight, interp, interp_jump, "mesh_scan")
    views: list = []
    cloud = filter_depth(pair_folder, scan_folder, cloud_ply, device=device, method=method, collect=views, **fusion_options)
    mesh, vol = mesh_views(views, voxel, trunc, min_weight, device, weight, interp, interp_jump)
    clean = (min_component, keep_largest) if int(min_component) > 0 or int(keep_largest) > 0 else None
    return dict(_finish(mesh, plyfilename, clean, smooth, simplify, placement, sample, surface_ply, fill), blocks=vol.n_blocks,
                cloud=cloud)


def clean_file(src_ply: str, dst_ply: str, min_component: int = 0, keep_largest: int = 0, device: str = "cuda",
               simplify: float = 0.0, placement: str = "quadric", sample: float = 0.0,
               surface_ply: Optional[str] = None, smooth: int = 0, smooth_lambda: float = 0.5, smooth_mu: float = -0.53,
               smooth_max_move: float = 0.0, fill_holes: int = 0) -> Dict[str, object]:
    """A saved mesh through :func:`clean_mesh`, then, with ``simplify`` > 0, through :func:`simplify_mesh`, and back into a file
    (``dst_ply`` may be ``src_ply``): what one runs while tuning the threshold or the cell, without the fusion.  With ``simplify``
    alone (both clean-up options at 0) the file goes through :func:`simplify_mesh` only, as in :func:`mesh_scan`.  ``sample`` > 0
    also writes the sampled surface of the mesh written to ``surface_ply``, as :func:`mesh_scan` does.  ``smooth`` > 0 sends it
    through :func:`smooth_mesh` before the simplification, as :func:`mesh_scan` does; with ``smooth`` alone, or with ``smooth`` and
    ``simplify``, the clean-up is skipped as with ``simplify`` alone.  ``fill_holes`` > 0 sends it through :func:`fill_holes` before
    the smoothing, as :func:`mesh_scan` does, and skips the clean-up in the same way when neither clean-up option is given.
    -> {"vertices", "faces", "mesh"[, "clean"][, "fill"][, "smooth"][, "simplify"][, "sample"]} as :func:`mesh_scan`."""
    simplify = _check_simplify(simplify, placement, "clean_file")
    sample = _check_sample(sample, surface_ply, "clean_file")
    smooth = _check_smooth(smooth, smooth_lambda, smooth_mu, smooth_max_move, "clean_file")
    fill = _check_fill(fill_holes, "clean_file")
    alone = simplify == 0 and smooth is None and fill == 0
    clean = (min_component, keep_largest) if alone or int(min_component) > 0 or int(keep_largest) > 0 else None
    return _finish(load_mesh(src_ply, device), dst_ply, clean, smooth, simplify, placement, sample, surface_ply, fill)


def format_mesh(info: Dict[str, object]) -> str:
    text = f"{info['vertices']} vertices, {info['faces']} faces"
    if "blocks" in info:
        text += f", {info['blocks']} blocks"
    if "clean" in info:
        c = info["clean"]
        text += (f"; removed {c['components'][0] - c['components'][1]} of {c['components'][0]} components and "
                 f"{c['faces'][0] - c['faces'][1]} of {c['faces'][0]} faces (the largest has {c['largest']})")
    if "fill" in info:
        h = info["fill"]
        text += (f"; filled {h['loops']} holes of at most {h['max_edges']} edges (the largest has {h['largest']}), border edges "
                 f"{h['border_edges'][0]} -> {h['border_edges'][1]}")
    if "smooth" in info:
        s = info["smooth"]
        text += (f"; smoothed {s['iterations']} iterations (lambda {s['lam']:g}, mu {s['mu']:g}): {s['boundary']} boundary, "
                 f"{s['isolated']} isolated vertices, largest move {s['max_move']:.6g}")
        if s.get("limit", 0) > 0:
            text += f", {s['clamped']} clamped to {s['limit']:g}"
    if "simplify" in info:
        s = info["simplify"]
        text += (f"; simplified {s['vertices'][0]} -> {s['vertices'][1]} vertices and {s['faces'][0]} -> {s['faces'][1]} faces "
                 f"({s['clusters']} clusters, {s['collapsed']} faces collapsed, {s['duplicates']} duplicates, {s['fallback']} fallbacks)")
    if "sample" in info:
        s = info["sample"]
        text += f"; surface sampled at {s['spacing']:g}: {s['points']} points (n up to {s['max_n']}, {s['skipped']} faces skipped)"
    return text


# ---------------------------------------------------------------------------------------------------------------------- CLI
def add_mesh_args(ap: argparse.ArgumentParser, required: bool = False) -> None:
    """The options of DESIGN §1.9, §1.11 to §1.15 and §1.20, shared with ``infer --fuse``."""
    ap.add_argument("--mesh_voxel", type=float, default=None, required=required, metavar="SIZE",
                    help="write <outdir>/<scan>_mesh.ply: a triangle mesh from a TSDF volume with this lattice spacing (world units)")
    ap.add_argument("--mesh_trunc", type=float, default=None, metavar="T",
                    help="--mesh_voxel: truncation distance, between 1 and 8 voxels (default 4 voxels)")
    ap.add_argument("--mesh_min_weight", type=int, default=2, metavar="N",
                    help="--mesh_voxel: views a lattice point needs before its cubes are meshed")
    ap.add_argument("--mesh_min_component", type=int, default=0, metavar="N",
                    help="--mesh_voxel: drop the connected components of the mesh with fewer than N faces (0: keep all)")
    ap.add_argument("--mesh_keep_largest", type=int, default=0, metavar="K",
                    help="--mesh_voxel: keep only the K components with the most faces (0: no limit)")
    ap.add_argument("--mesh_simplify", type=float, default=None, metavar="CELL",
                    help="--mesh_voxel: simplify the mesh before it is written: one vertex per cell of this side (world units, the "
                         "cells of --merge_voxel), faces that collapse or repeat dropped")
    ap.add_argument("--mesh_simplify_placement", default="quadric", choices=list(PLACEMENTS),
                    help="--mesh_simplify: a cell's vertex at the minimiser of its faces' quadric error (edges and corners "
                         "survive) or at the mean of its vertices")
    ap.add_argument("--mesh_fill_holes", type=int, default=None, metavar="N",
                    help=f"--mesh_voxel: close the holes of the mesh whose rim has at most N border edges (3..{MAX_FILL_EDGES}), after "
                         "the clean-up and before the smoothing: one face for a hole of 3, else a fan around the mean of the rim")
    ap.add_argument("--mesh_smooth", type=int, default=None, metavar="ITER",
                    help="--mesh_voxel: smooth the mesh before it is simplified and written: ITER iterations (1..1000) of the "
                         "lambda|mu filter, which moves the vertices and nothing else")
    ap.add_argument("--mesh_smooth_lambda", type=float, default=None, metavar="L",
                    help="--mesh_smooth: the step towards the neighbours' mean, in (0, 1] (default 0.5)")
    ap.add_argument("--mesh_smooth_mu", type=float, default=None, metavar="M",
                    help="--mesh_smooth: the step back that keeps the volume, in [-1, 0] (default -0.53; 0: plain Laplacian)")
    ap.add_argument("--mesh_smooth_max_move", type=float, default=None, metavar="D",
                    help="--mesh_smooth: no vertex ends farther than D (world units) from where it was (default: no limit)")
    ap.add_argument("--mesh_sample", type=float, default=None, metavar="SPACING",
                    help="--mesh_voxel: also write <outdir>/<scan>_surface.ply, the surface of the mesh written as a cloud: the "
                         "centroids of every face's sub-triangles with edges of at most SPACING (world units)")
    ap.add_argument("--mesh_weight", default="one", choices=list(WEIGHT_MODES),
                    help="--mesh_voxel: what a kept pixel weighs in the volume: one; angle, the cosine between its viewing ray and "
                         "the normal of its depth map; conf, its last-stage confidence; angle_conf, their product")
    ap.add_argument("--mesh_interp", action="store_true",
                    help="--mesh_voxel: interpolate the depth between the four pixels around a projection (in inverse depth) where "
                         "they are kept and close in depth, instead of taking the nearest pixel's")
    ap.add_argument("--mesh_interp_jump", type=float, default=None, metavar="J",
                    help="--mesh_interp: the largest relative depth difference among the four pixels (default 0.05)")


def check_weight_args(ap: argparse.ArgumentParser, args, allowed: bool) -> float:
    """ap.error for --mesh_weight, --mesh_interp or --mesh_interp_jump where no volume is integrated (``allowed`` false), for a
    jump without --mesh_interp and for one that is not positive -> the jump (0.05 unless given)."""
    given = [name for name, on in (("--mesh_weight", args.mesh_weight != "one"), ("--mesh_interp", args.mesh_interp),
                                   ("--mesh_interp_jump", args.mesh_interp_jump is not None)) if on]
    if given and not allowed:
        ap.error(f"{', '.join(given)}: these options weigh the views of --mesh_voxel: give --mesh_voxel SIZE (a saved mesh of "
                 "--from_mesh is not integrated again)")
    if args.mesh_interp_jump is None:
        return 0.05
    if not args.mesh_interp:
        ap.error("--mesh_interp_jump belongs to --mesh_interp")
    try:
        return _positive(args.mesh_interp_jump, "--mesh_interp_jump")
    except ValueError as e:
        ap.error(str(e))


def check_clean_args(ap: argparse.ArgumentParser, args, allowed: bool) -> None:
    """ap.error for a negative clean-up option, a non-positive --mesh_simplify or --mesh_sample, a --mesh_fill_holes outside its
    range, bad --mesh_smooth values, one of --mesh_smooth's options without it, or for any of them given where no mesh is made
    (``allowed`` false)."""
    if args.mesh_min_component < 0 or args.mesh_keep_largest < 0:
        ap.error(f"--mesh_min_component and --mesh_keep_largest must be >= 0, got {args.mesh_min_component} and "
                 f"{args.mesh_keep_largest}")
    if not allowed and (args.mesh_min_component or args.mesh_keep_largest):
        ap.error("--mesh_min_component and --mesh_keep_largest clean the mesh of --mesh_voxel: give --mesh_voxel SIZE as well")
    for option, does in (("mesh_simplify", "simplifies"), ("mesh_sample", "samples")):
        value = getattr(args, option)
        if value is None:
            continue
        try:
            _positive(value, "--" + option)
        except ValueError as e:
            ap.error(str(e))
        if not allowed:
            ap.error(f"--{option} {does} the mesh of --mesh_voxel: give --mesh_voxel SIZE (or, in mesh, --from_mesh FILE) as well")
    if args.mesh_fill_holes is not None:
        try:
            check_fill(args.mesh_fill_holes, "--mesh_fill_holes")
        except ValueError as e:
            ap.error(str(e))
        if not allowed:
            ap.error("--mesh_fill_holes fills the holes of the mesh of --mesh_voxel: give --mesh_voxel SIZE (or, in mesh, --from_mesh "
                     "FILE) as well")
    given = [name for name in ("mesh_smooth", "mesh_smooth_lambda", "mesh_smooth_mu", "mesh_smooth_max_move")
             if getattr(args, name) is not None]
    if given and not allowed:
        ap.error(f"--{', --'.join(given)}: these options smooth the mesh of --mesh_voxel: give --mesh_voxel SIZE (or, in mesh, "
                 "--from_mesh FILE) as well")
    if given and args.mesh_smooth is None:
        ap.error(f"--{', --'.join(given)} belong to --mesh_smooth ITER")
    if given:
        try:
            check_smooth(args.mesh_smooth, *smooth_args(args)[1:], what="--mesh_smooth")
        except ValueError as e:
            ap.error(str(e))


def smooth_args(args):
    """The parsed --mesh_smooth options -> (smooth, smooth_lambda, smooth_mu, smooth_max_move) for :func:`mesh_scan`: 0 iterations
    without --mesh_smooth, the defaults for what was not given."""
    return (args.mesh_smooth or 0, 0.5 if args.mesh_smooth_lambda is None else args.mesh_smooth_lambda,
            -0.53 if args.mesh_smooth_mu is None else args.mesh_smooth_mu,
            0.0 if args.mesh_smooth_max_move is None else args.mesh_smooth_max_move)


def main(argv=None) -> Dict[str, Dict[str, object]]:
    from .fusion import DYN_DIST_BASE, DYN_REL_BASE, _floats
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--testpath", default=None, help="the scenes: <testpath>/<scan>/pair.txt (not needed with --from_mesh)")
    ap.add_argument("--outdir", required=True, help="the infer output folder: <outdir>/<scan>/{depth_est,confidence,cams,images}")
    ap.add_argument("--testlist", required=True, help="text file with one scan name per line")
    ap.add_argument("--filter_method", default="normal", choices=["normal", "dynamic", "gipuma"])
    ap.add_argument("--conf", default="0.0,0.0,0.0", help="per-stage confidence thresholds")
    ap.add_argument("--thres_view", type=int, default=3, help="normal: consistent views a pixel needs")
    ap.add_argument("--thres_disp", type=float, default=1.0, help="normal: re-projection distance threshold in pixels")
    ap.add_argument("--dyn_dist_base", type=float, default=DYN_DIST_BASE, help="dynamic: pixels per level")
    ap.add_argument("--dyn_rel_base", type=float, default=DYN_REL_BASE, help="dynamic: relative depth difference per level")
    ap.add_argument("--dyn_views", default="2,10", help="dynamic: n_min,n_max")
    ap.add_argument("--device", default="cuda")
    add_mesh_args(ap)
    ap.add_argument("--from_mesh", default=None, metavar="FILE",
                    help="instead of --mesh_voxel: clean this saved mesh ({scan} is replaced) with --mesh_min_component / "
                         "--mesh_keep_largest, fill its holes with --mesh_fill_holes, smooth it with --mesh_smooth, simplify it with --mesh_simplify, and write <outdir>/<scan>_mesh.ply, without any "
                         "fusion")
    args = ap.parse_args(argv)
    if args.mesh_voxel is None and args.from_mesh is None and args.mesh_sample is not None:
        ap.error("--mesh_sample samples the mesh of --mesh_voxel: give --mesh_voxel SIZE or --from_mesh FILE as well")
    if (args.mesh_voxel is None) == (args.from_mesh is None):
        ap.error("give either --mesh_voxel SIZE (fuse and mesh) or --from_mesh FILE (clean a saved mesh)")
    check_clean_args(ap, args, True)
    interp_jump = check_weight_args(ap, args, args.from_mesh is None)
    if args.from_mesh is None and args.testpath is None:
        ap.error("--testpath is required with --mesh_voxel")
    if args.filter_method == "gipuma":
        ap.error("--mesh_voxel is not implemented for --filter_method gipuma (its fused point has no single depth map); "
                 "use normal or dynamic")
    scans = read_testlist(args.testlist)
    out = {}
    if args.from_mesh is not None:
        for scan in scans:
            out[scan] = clean_file(args.from_mesh.format(scan=scan), os.path.join(args.outdir, f"{scan}_mesh.ply"),
                                   args.mesh_min_component, args.mesh_keep_largest, device=args.device,
                                   simplify=args.mesh_simplify or 0.0, placement=args.mesh_simplify_placement,
                                   sample=args.mesh_sample or 0.0, surface_ply=os.path.join(args.outdir, f"{scan}_surface.ply"),
                                   **dict(zip(SMOOTH_KEYS, smooth_args(args))), fill_holes=args.mesh_fill_holes or 0)
            print(f"{scan}_mesh.ply: {format_mesh(out[scan])}", flush=True)
        return out
    for scan in scans:
        info = mesh_scan(os.path.join(args.testpath, scan), os.path.join(args.outdir, scan),
                         os.path.join(args.outdir, f"{scan}_mesh.ply"), args.mesh_voxel, args.mesh_trunc, args.mesh_min_weight,
                         method=args.filter_method, device=args.device, min_component=args.mesh_min_component,
                         keep_largest=args.mesh_keep_largest, simplify=args.mesh_simplify or 0.0,
                         placement=args.mesh_simplify_placement, sample=args.mesh_sample or 0.0,
                         surface_ply=os.path.join(args.outdir, f"{scan}_surface.ply"), weight=args.mesh_weight,
                         interp=args.mesh_interp, interp_jump=interp_jump, **dict(zip(SMOOTH_KEYS, smooth_args(args))),
                         fill_holes=args.mesh_fill_holes or 0,
                         conf=_floats(args.conf, 3, "--conf"),
                         thres_disp=args.thres_disp, thres_view=args.thres_view, dist_base=args.dyn_dist_base,
                         rel_base=args.dyn_rel_base, n_views=tuple(int(v) for v in _floats(args.dyn_views, 2, "--dyn_views")))
        out[scan] = info
        print(f"{scan}_mesh.ply: {format_mesh(info)}", flush=True)
    return out


if __name__ == "__main__":
    main()
