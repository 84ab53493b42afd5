"""A mesh textured from the images of its scan, on the GPU: a texture atlas and an OBJ that Blender or MeshLab opens (DESIGN §1.17;
the rule is in include/cds_mvsnet_hip.h).

Every face takes its colour from one view, the one in which the rasteriser of §1.10 shows most of it, and owns one square cell of
the atlas, sized from its longest edge in that view.  The cells are packed along a Z-order curve, every texel of a cell is the
bilinear sample of the view's image at the projection of its surface point, and faces that no view sees keep their interpolated
vertex colours.  The output is a function of the input alone.  The hot paths are the kernels of ``csrc/mesh_texture.hip``
(``cds_texture_votes``, ``cds_texture_best``, ``cds_texture_cells``, ``cds_texture_place``, ``cds_texture_fill``) behind
``render.render_mesh``; torch sorts the cell sizes and sums the units between two launches.  There is no CPU path.

``level=ITER`` (``--texture_level ITER``) levels the seams between faces that take their colour from different views (DESIGN
§1.19, rules L1-L6 of the header): an additive correction per (vertex, view), a per-view offset found by least squares from the
integer pair table of ``cds_texture_level_pairs`` and ITER damped Jacobi steps of ``cds_texture_level_step``, interpolated over
each face by ``cds_texture_fill_level``.  Without it nothing new runs.

    python -m cds_mvsnet_amd.texture --testpath <scenes> --outdir <out> --testlist <list> [--mesh "<out>/{scan}_mesh.ply"]
        [--texture_scale S] [--texture_max_cell C] [--texture_max_size N] [--texture_min_px P]
        [--texture_level ITER [--texture_level_lambda L]]

textures ``<out>/<scan>_mesh.ply`` from ``<out>/<scan>/images/%08d.jpg`` with the cameras of ``<out>/<scan>/cams`` for the views of
``<testpath>/<scan>/pair.txt`` and writes ``<out>/<scan>_textured.{obj,mtl,png}``.
``infer ... --fuse --mesh_voxel SIZE --texture`` does the same right after the mesh is written.
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from .mesh import check_mesh_device, check_mesh_layout, load_mesh
from .mvs_io import ScanFolder, read_pair_file, read_testlist
from .render import CAM_DOUBLES, MAX_CHUNK, camera_table, render_mesh

Tensor = torch.Tensor

MAX_CELL = 4096                # CDS_TEXTURE_MAX_CELL
MAX_SIZE = 32768               # CDS_TEXTURE_MAX_SIZE
DEFAULTS = dict(scale=1.0, max_cell=256, max_size=16384, min_px=1, level=0, level_lambda=0.1)
LEVEL_MAX_VIEWS = 512          # CDS_TEXTURE_LEVEL_MAX_VIEWS: rule L3 keeps a dense V x V table
LEVEL_RIDGE = 2.0 ** -10       # rule L3
VOTE_RUNS = 1                  # cds_texture_votes: one add per run of equal faces (profiles/mesh_texture.md)
FILL_PER_UNIT = 1              # cds_texture_fill: one thread per 4 x 4 unit, one search for its 16 texels (profiles/mesh_texture.md)


def _is_pow2(n: int) -> bool:
    return n >= 1 and n & (n - 1) == 0


def check_level_args(level, level_lambda, what: str = "texture_mesh") -> Tuple[int, float]:
    """-> (level, level_lambda); ValueError unless level is an integer >= 0 and level_lambda finite and > 0."""
    if isinstance(level, bool) or int(level) != level or int(level) < 0 or int(level) >= 2 ** 31:
        raise ValueError(f"{what}: level must be a number of iterations >= 0, got {level}")
    level_lambda = float(level_lambda)
    if not (level_lambda > 0 and level_lambda < float("inf")):
        raise ValueError(f"{what}: level_lambda must be finite and > 0, got {level_lambda}")
    return int(level), level_lambda


def check_texture_args(scale, max_cell, max_size, min_px, what: str = "texture_mesh", level=0,
                       level_lambda=0.1) -> Tuple[float, int, int, int]:
    """-> (scale, max_cell, max_size, min_px); ValueError unless scale is finite and > 0, max_cell a power of two in 4..4096,
    max_size in 4..32768 and min_px >= 1, and unless level and level_lambda pass :func:`check_level_args`."""
    check_level_args(level, level_lambda, what)
    scale = float(scale)
    if not (scale > 0 and scale < float("inf")):
        raise ValueError(f"{what}: scale must be finite and > 0, got {scale}")
    max_cell, max_size, min_px = int(max_cell), int(max_size), int(min_px)
    if not (4 <= max_cell <= MAX_CELL and _is_pow2(max_cell)):
        raise ValueError(f"{what}: max_cell must be a power of two in 4..{MAX_CELL}, got {max_cell}")
    if not 4 <= max_size <= MAX_SIZE:
        raise ValueError(f"{what}: max_size must lie in 4..{MAX_SIZE}, got {max_size}")
    if not 1 <= min_px < 2 ** 31:
        raise ValueError(f"{what}: min_px must be >= 1, got {min_px}")
    return scale, max_cell, max_size, min_px


def atlas_size(total: int, max_size: int = MAX_SIZE, what: str = "texture_mesh") -> Tuple[int, int]:
    """Rule 4: the units of 4 x 4 texels that the cells take -> (H, W).  W is the smallest power of two >= 4 with
    (W / 4)^2 >= total, H = W / 2 when the cells fit the first half of the curve.  ValueError when W > max_size."""
    total = int(total)
    if total < 1:
        raise ValueError(f"{what}: an atlas of {total} units")
    w = 4
    while (w // 4) ** 2 < total:
        w *= 2
    if w > int(max_size):
        raise ValueError(f"{what}: the cells take {total} units of 4 x 4 texels, an atlas {w} texels wide, at most {int(max_size)}: "
                         "lower --texture_scale or simplify the mesh further")
    return (w // 2 if 2 * total <= (w // 4) ** 2 else w), w


def _view_groups(images, cams, what: str):
    """images and cams of texture_mesh -> [(images [V,h,w,3], cams [V,2,4,4])], one entry per image size (ValueError)."""
    single = isinstance(images, torch.Tensor)
    if single != isinstance(cams, torch.Tensor) or (not single and (not isinstance(images, (list, tuple)) or not isinstance(
            cams, (list, tuple)) or len(images) != len(cams))):
        raise ValueError(f"{what}: images and cams must be two tensors, or two lists of equally many tensors, one pair per image size")
    groups = [(images, cams)] if single else list(zip(images, cams))
    for img, cam in groups:
        if not isinstance(img, torch.Tensor) or img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8:
            raise ValueError(f"{what}: images must be a uint8 [V,h,w,3] tensor, got {getattr(img, 'dtype', type(img))} "
                             f"{tuple(getattr(img, 'shape', ()))}")
        v, h, w = (int(x) for x in img.shape[:3])
        if not isinstance(cam, torch.Tensor) or cam.dim() != 4 or tuple(cam.shape) != (v, 2, 4, 4):
            raise ValueError(f"{what}: cams must be [{v},2,4,4], one per image, got {tuple(getattr(cam, 'shape', ()))}")
        if h < 1 or w < 1 or h * w >= 2 ** 31:
            raise ValueError(f"{what}: images of {h} x {w}")
    return groups


# ----------------------------------------------------------------------------------------------------------------- levelling
def level_offsets(cnt, dsum, n_label) -> np.ndarray:
    """Rule L3 on the host: cnt int64 [V,V] and dsum int64 [V,V,3] as cds_texture_level_pairs left them (entries with a < b),
    n_label int64 [V]: the nodes of every label -> o fp64 [V,3], the solution of the normal equations, per channel."""
    cnt, dsum = np.asarray(cnt, np.int64), np.asarray(dsum, np.int64)
    v = cnt.shape[0]
    up = np.triu(cnt, 1).astype(np.float64)
    sym = up + up.T
    a = np.diag(sym.sum(1) + LEVEL_RIDGE * np.maximum(np.asarray(n_label, np.int64), 1).astype(np.float64)) - sym
    o = np.zeros((v, 3), np.float64)
    for ch in range(3):
        d = np.triu(dsum[:, :, ch], 1).astype(np.float64) / 256.0       # cnt[a][b] D[a][b]
        o[:, ch] = np.linalg.solve(a, d.sum(0) - d.sum(1))
    return o


def _seam_jump(sample: Tensor, ok: Tensor, vertex: Tensor, g: Tensor, longest: int) -> Tensor:
    """The sum over the ok pairs of one vertex and the channels of |(s_i + g_i) - (s_j + g_j)|, on the device (reporting only)."""
    t = sample + g
    total = torch.zeros((), dtype=torch.float64, device=sample.device)
    for d in range(1, longest):
        pair = (vertex[d:] == vertex[:-d]) & ok[d:] & ok[:-d]
        total = total + ((t[d:] - t[:-d]).abs().sum(1) * pair).sum()
    return total


def level_pair_table(node_key: Tensor, sample: Tensor, ok: Tensor, n_views: int):
    """The table of rule L3 from the nodes of :func:`texture_mesh`'s "level" -> (table int64 [V,V,4] = cnt, dsum[3] on the device,
    span int32 [N,2]: the first node of every node's vertex and the number of its nodes, the longest span as a tensor [1])."""
    dev, n = node_key.device, int(node_key.numel())
    table = torch.zeros((n_views, n_views, 4), dtype=torch.int64, device=dev)
    if n == 0:
        return table, torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    _, which, count = torch.unique_consecutive(node_key // n_views, return_inverse=True, return_counts=True)
    span = torch.stack([(torch.cumsum(count, 0) - count)[which], count[which]], 1).to(torch.int32).contiguous()
    with torch.cuda.device(dev):
        check(_lib.load().cds_texture_level_pairs(sample.data_ptr(), ok.data_ptr(), node_key.data_ptr(), span.data_ptr(), n, n_views,
                                                  table.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "cds_texture_level_pairs")
    return table, span, count.max().reshape(1)


def level_nodes(faces: Tensor, view: Tensor, n_views: int, what: str = "texture_mesh") -> Dict[str, Tensor]:
    """Rule L1, by torch's sort: faces int32 [NF,3] and view int32 [NF] on the device -> {"node_key" int64 [N], "corner_node" int32
    [NF,3], "corner_list" int64: the corners 3 f + k of node 0, ascending, then those of node 1, ..., "corner_start" int64 [N+1]}."""
    dev, nf = faces.device, int(faces.shape[0])
    seen = (view >= 0)[:, None].expand(nf, 3).reshape(-1)
    corners = torch.nonzero(seen).reshape(-1)                         # ascending
    keys = (faces.to(torch.int64) * n_views + view.to(torch.int64)[:, None]).reshape(-1)[corners]
    node_key, inverse = torch.unique(keys, sorted=True, return_inverse=True)
    n = int(node_key.numel())
    if n >= 2 ** 31:
        raise ValueError(f"{what}: {n} (vertex, view) nodes, at most 2^31 - 1")
    corner_node = torch.full((3 * nf,), -1, dtype=torch.int32, device=dev)
    corner_node[corners] = inverse.to(torch.int32)
    corner_start = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    corner_start[1:] = torch.cumsum(torch.bincount(inverse, minlength=n), 0)
    return {"node_key": node_key, "corner_node": corner_node.reshape(nf, 3),
            "corner_list": corners[torch.sort(inverse, stable=True).indices].contiguous(), "corner_start": corner_start}


def _level(lib, stream, vert, nv, faces, nf, tab, pixels, views, v, view, level, level_lambda, what):
    """Rules L1-L5 -> (the "level" dict of texture_mesh, pairs, the two jump sums as a device tensor [2])."""
    dev = vert.device
    nodes = level_nodes(faces, view, v, what)
    node_key, corner_node, corner_list, corner_start = (nodes[k] for k in ("node_key", "corner_node", "corner_list", "corner_start"))
    n = int(node_key.numel())
    vertex, label = node_key // v, node_key % v
    sample = torch.empty((n, 3), dtype=torch.float64, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    check(lib.cds_texture_level_samples(vert.data_ptr(), nv, tab.data_ptr(), pixels.data_ptr(), int(pixels.numel()), views.data_ptr(),
                                        v, node_key.data_ptr(), n, sample.data_ptr(), ok.data_ptr(), stream), "cds_texture_level_samples")
    table, span, longest = level_pair_table(node_key, sample, ok, v)
    # rule L3: the one read of levelling
    host = torch.cat([table.reshape(-1), torch.bincount(label, minlength=v), longest]).cpu().numpy()
    pair = host[:4 * v * v].reshape(v, v, 4)
    offsets = torch.from_numpy(level_offsets(pair[:, :, 0], pair[:, :, 1:], host[4 * v * v:4 * v * v + v])).to(dev)
    g = offsets[label].contiguous() if n else torch.zeros((0, 3), dtype=torch.float64, device=dev)     # rule L4
    other = torch.empty_like(g)
    for _ in range(level):                                            # rule L5: nothing is read on the host
        check(lib.cds_texture_level_step(sample.data_ptr(), ok.data_ptr(), span.data_ptr(), corner_start.data_ptr(),
                                         corner_list.data_ptr(), int(corner_list.numel()), corner_node.data_ptr(), n, nf, v,
                                         level_lambda, g.data_ptr(), other.data_ptr(), stream), "cds_texture_level_step")
        g, other = other, g
    okb = ok != 0
    jumps = torch.stack([_seam_jump(sample, okb, vertex, torch.zeros_like(g), int(host[-1])),
                         _seam_jump(sample, okb, vertex, g, int(host[-1]))])
    out = {"node_key": node_key, "corner_node": corner_node, "sample": sample, "ok": ok, "offsets": offsets, "g": g}
    return out, int(pair[:, :, 0].sum()), jumps


def texture_mesh(mesh_dict: Dict[str, Tensor], images, cams, scale: float = 1.0, max_cell: int = 256, max_size: int = 16384,
                 min_px: int = 1, chunk: int = 8, level: int = 0, level_lambda: float = 0.1):
    """``mesh_dict`` as the mesh stage returns it (vertices float32 [NV,3], colors uint8 [NV,3], faces int32 [NF,3], on one ROCm
    device); ``images`` uint8 [V,h,w,3] on that device; ``cams`` [V,2,4,4] on any device, as ``render.render_mesh`` takes them.
    For views of several image sizes, ``images`` and ``cams`` are two lists with one such pair per size; the views are numbered
    through the lists in their order.
    ``scale``: texels per pixel of a face's longest edge in its view; ``max_cell``: the largest cell, a power of two;
    ``max_size``: the widest atlas (ValueError beyond); a face needs ``min_px`` pixels in its best view to take its colour from
    it; ``chunk`` views are rendered at a time, and the result does not depend on it.
    -> ({"atlas" uint8 [H,W,3], "uv" int32 [NF,3,2]: the texel coordinates of the three corners (x, y), "view" int32 [NF] (-1: no
    view sees the face), "cell" int32 [NF,3]: (x0, y0, c)} on that device; info: {"H", "W", "faces", "unseen", "units": (used, of
    the atlas), "views"}).  An empty mesh gives an empty atlas [0,0,3]; so do zero views, with view -1 and cell 0 for every face:
    neither launches anything.
    ``level`` > 0: the seams are levelled with that many iterations of rule L5 at the smoothness weight
    ``level_lambda``; uv, view and cell are what they are without it.  The result gains "level": {"node_key" int64 [N],
    "corner_node" int32 [NF,3], "sample" float64 [N,3], "ok" uint8 [N], "offsets" float64 [V,3], "g" float64 [N,3]} on the device,
    and info "seam": (the seam pairs, their mean colour jump before, and after levelling).  ValueError beyond 512 views."""
    what = "texture_mesh"
    vert, col, faces = mesh_dict["vertices"], mesh_dict["colors"], mesh_dict["faces"]
    nv, nf = check_mesh_layout(vert, col, faces, what), int(faces.shape[0])
    if col is None:
        raise ValueError(f"{what}: the mesh needs colors, a uint8 [{nv},3] tensor")
    groups = _view_groups(images, cams, what)
    chunk = int(chunk)
    if not (1 <= chunk <= MAX_CHUNK):
        raise ValueError(f"{what}: chunk must lie in 1..{MAX_CHUNK}, got {chunk}")
    scale, max_cell, max_size, min_px = check_texture_args(scale, max_cell, max_size, min_px, what)
    level, level_lambda = check_level_args(level, level_lambda, what)
    tab = torch.cat([camera_table(cam) for _, cam in groups]) if groups else torch.zeros((0, CAM_DOUBLES), dtype=torch.float64)
    dev = check_mesh_device(vert, col, faces, what)
    for img, _ in groups:
        if not img.is_cuda or img.device != dev:
            raise RuntimeError(f"{what}: images must be on {dev}; there is no CPU fallback")
    v = int(tab.shape[0])
    if level and v > LEVEL_MAX_VIEWS:
        raise ValueError(f"{what}: levelling keeps a table of views x views: at most {LEVEL_MAX_VIEWS} views, got {v}")
    out = {"atlas": torch.zeros((0, 0, 3), dtype=torch.uint8, device=dev), "uv": torch.zeros((nf, 3, 2), dtype=torch.int32, device=dev),
           "view": torch.full((nf,), -1, dtype=torch.int32, device=dev), "cell": torch.zeros((nf, 3), dtype=torch.int32, device=dev)}
    info = {"H": 0, "W": 0, "faces": nf, "unseen": nf, "units": (0, 0), "views": v}
    if nf == 0 or v == 0:
        if level:
            out["level"] = {"node_key": torch.zeros(0, dtype=torch.int64, device=dev),
                            "corner_node": torch.full((nf, 3), -1, dtype=torch.int32, device=dev),
                            "sample": torch.zeros((0, 3), dtype=torch.float64, device=dev), "ok": torch.zeros(0, dtype=torch.uint8, device=dev),
                            "offsets": torch.zeros((v, 3), dtype=torch.float64, device=dev),
                            "g": torch.zeros((0, 3), dtype=torch.float64, device=dev)}
            info["seam"] = (0, 0.0, 0.0)
        return out, info
    vert, col, faces = vert.contiguous(), col.contiguous(), faces.contiguous()
    groups = [(img.contiguous(), cam) for img, cam in groups if img.shape[0] > 0]
    # the images as one run of bytes and the table of its views: byte offset, h, w
    pixels = groups[0][0].reshape(-1) if len(groups) == 1 else torch.cat([img.reshape(-1) for img, _ in groups])
    rows, off = [], 0
    for img, _ in groups:
        n, h, w = (int(x) for x in img.shape[:3])
        rows += [(off + 3 * h * w * k, h, w) for k in range(n)]
        off += 3 * h * w * n
    views = torch.tensor(rows, dtype=torch.int64).to(dev)
    tab = tab.to(dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        key = torch.zeros(nf, dtype=torch.int64, device=dev)
        votes = torch.empty((min(chunk, v), nf), dtype=torch.int32, device=dev)
        first = 0                                                     # the number of the group's first view
        for img, cam in groups:
            gv, h, w = (int(x) for x in img.shape[:3])
            for v0 in range(0, gv, chunk):
                n = min(chunk, gv - v0)
                maps = render_mesh(vert, faces, cam[v0:v0 + n], h, w, chunk=chunk)                   # rule 1: §1.10, unchanged
                votes.zero_()
                check(lib.cds_texture_votes(maps["face"].data_ptr(), maps["valid"].data_ptr(), n, h, w, nf, votes.data_ptr(),
                                            VOTE_RUNS, stream), "cds_texture_votes")
                check(lib.cds_texture_best(votes.data_ptr(), nf, n, first + v0, key.data_ptr(), stream), "cds_texture_best")
            first += gv
        check(lib.cds_texture_cells(vert.data_ptr(), nv, faces.data_ptr(), nf, tab.data_ptr(), v, key.data_ptr(), min_px, scale,
                                    max_cell, out["view"].data_ptr(), out["cell"].data_ptr(), stream), "cds_texture_cells")
        # rule 4 between two launches: the sort by size and the prefix sums of the units
        c = out["cell"][:, 2].to(torch.int64)
        order = torch.sort(-c, stable=True).indices
        units = (c[order] >> 2) ** 2
        ends = torch.cumsum(units, 0)
        counts = torch.stack([ends[-1], (out["view"] < 0).sum()])
        if level:
            # before the read below, so that the report of the seams travels with it: levelling itself reads only its pair table
            out["level"], pairs, jumps = _level(lib, stream, vert, nv, faces, nf, tab, pixels, views, v, out["view"], level,
                                                level_lambda, what)
            counts = torch.cat([counts, jumps.view(torch.int64)])
        counts = counts.cpu()                                         # the one read
        total, unseen = int(counts[0]), int(counts[1])
        if level:
            before, after = (float(x) / (3 * pairs) if pairs else 0.0 for x in counts[2:].view(torch.float64))
            info["seam"] = (pairs, before, after)
        ah, aw = atlas_size(total, max_size, what)
        starts = ends - units
        check(lib.cds_texture_place(order.data_ptr(), starts.data_ptr(), nf, total, max_cell, out["cell"].data_ptr(),
                                    out["uv"].data_ptr(), stream), "cds_texture_place")
        out["atlas"] = torch.empty((ah, aw, 3), dtype=torch.uint8, device=dev)
        fill = (vert.data_ptr(), col.data_ptr(), nv, faces.data_ptr(), nf, tab.data_ptr(), pixels.data_ptr(), int(pixels.numel()),
                views.data_ptr(), v, out["view"].data_ptr(), out["cell"].data_ptr(), order.data_ptr(), starts.data_ptr(), total,
                max_cell, ah, aw, out["atlas"].data_ptr(), FILL_PER_UNIT)
        if level:
            lv = out["level"]
            check(lib.cds_texture_fill_level(*fill, lv["corner_node"].data_ptr(), lv["g"].data_ptr(), int(lv["g"].shape[0]), stream),
                  "cds_texture_fill_level")
        else:
            check(lib.cds_texture_fill(*fill, stream), "cds_texture_fill")
    info.update(H=ah, W=aw, unseen=unseen, units=(total, (ah // 4) * (aw // 4)))
    return out, info


def format_texture(info: Dict[str, object]) -> str:
    used, room = info["units"]
    line = (f"atlas {info['W']} x {info['H']}, {100.0 * used / room if room else 0.0:.1f} % of its units used, {info['faces']} faces from "
            f"{info['views']} views, {100.0 * info['unseen'] / info['faces'] if info['faces'] else 0.0:.2f} % unseen")
    if "seam" in info:
        pairs, before, after = info["seam"]
        line += f", {pairs} seam pairs levelled: mean jump {before:.2f} -> {after:.2f} levels"
    return line


# -------------------------------------------------------------------------------------------------------------------- files
def _host(t) -> np.ndarray:
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def write_textured_obj(prefix: str, mesh, out) -> None:
    """``<prefix>.obj``, ``<prefix>.mtl`` and ``<prefix>.png`` from a mesh dict (vertices, faces) and the result of
    :func:`texture_mesh` (tensors or arrays).  ``v`` with %.9g, so float32 positions read back by their bits; three ``vt`` per
    face, (x / W, 1 - y / H): W and H are powers of two, so the values are exact; ``f a/ta b/tb c/tc``, 1-based."""
    vert, faces = _host(mesh["vertices"]).astype(np.float32), _host(mesh["faces"]).astype(np.int64)
    atlas, uv = np.ascontiguousarray(_host(out["atlas"])), _host(out["uv"]).astype(np.int64)
    if atlas.ndim != 3 or atlas.shape[2] != 3 or atlas.dtype != np.uint8 or atlas.shape[0] < 1 or atlas.shape[1] < 1:
        raise ValueError(f"write_textured_obj: the atlas must be a uint8 [H,W,3] image, got {atlas.dtype} {atlas.shape}")
    if uv.shape != (len(faces), 3, 2):
        raise ValueError(f"write_textured_obj: uv must be [{len(faces)},3,2], got {uv.shape}")
    ah, aw = atlas.shape[:2]
    name = os.path.basename(prefix)
    from PIL import Image
    Image.fromarray(atlas).save(prefix + ".png")
    with open(prefix + ".mtl", "w") as f:
        f.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    tu, tv = uv[..., 0].reshape(-1) / float(aw), 1.0 - uv[..., 1].reshape(-1) / float(ah)
    with open(prefix + ".obj", "w") as f:
        f.write(f"mtllib {name}.mtl\nusemtl {name}\n")
        f.write("".join("v %.9g %.9g %.9g\n" % (float(p[0]), float(p[1]), float(p[2])) for p in vert))
        f.write("".join("vt %.17g %.17g\n" % (a, b) for a, b in zip(tu.tolist(), tv.tolist())))
        f.write("".join("f %d/%d %d/%d %d/%d\n" % (a + 1, 3 * k + 1, b + 1, 3 * k + 2, c + 1, 3 * k + 3)
                        for k, (a, b, c) in enumerate(faces.tolist())))


def read_textured_obj(path: str):
    """An OBJ of :func:`write_textured_obj` -> {"vertices" float32 [NV,3], "faces" int32 [NF,3], "vt" float64 [NT,2], "face_vt" int32
    [NF,3], "atlas" uint8 [H,W,3] (the image its material names), "mtllib", "usemtl"}."""
    v, vt, fv, ft = [], [], [], []
    mtllib = usemtl = None
    with open(path) as f:
        for line in f:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([np.float32(x) for x in p[1:4]])
            elif p[0] == "vt":
                vt.append([float(x) for x in p[1:3]])
            elif p[0] == "f":
                pairs = [q.split("/") for q in p[1:4]]
                fv.append([int(q[0]) - 1 for q in pairs])
                ft.append([int(q[1]) - 1 for q in pairs])
            elif p[0] == "mtllib":
                mtllib = p[1]
            elif p[0] == "usemtl":
                usemtl = p[1]
    atlas = None
    if mtllib is not None:
        folder = os.path.dirname(path)
        with open(os.path.join(folder, mtllib)) as f:
            maps = [ln.split()[1] for ln in f if ln.startswith("map_Kd")]
        if maps:
            from PIL import Image
            atlas = np.asarray(Image.open(os.path.join(folder, maps[0])).convert("RGB"))
    return {"vertices": np.asarray(v, np.float32).reshape(-1, 3), "faces": np.asarray(fv, np.int32).reshape(-1, 3),
            "vt": np.asarray(vt, np.float64).reshape(-1, 2), "face_vt": np.asarray(ft, np.int32).reshape(-1, 3), "atlas": atlas,
            "mtllib": mtllib, "usemtl": usemtl}


# -------------------------------------------------------------------------------------------------------------------- scans
def texture_scan(scan_out_folder: str, mesh_ply, pair_folder: str, prefix: str, scale: float = 1.0, max_cell: int = 256,
                 max_size: int = 16384, min_px: int = 1, device: str = "cuda", chunk: int = 8, level: int = 0,
                 level_lambda: float = 0.1) -> Dict[str, object]:
    """Texture a mesh from the views of ``<pair_folder>/pair.txt``, in that order: the images ``<scan_out_folder>/images/%08d.jpg``
    with the cameras of ``<scan_out_folder>/cams/%08d_cam.txt``, and write ``<prefix>.{obj,mtl,png}``.  ``mesh_ply``: a file of
    ``mesh.write_mesh_ply``, or the mesh dict of the mesh stage on the device.  The views are grouped by image size as
    ``render.render_scan`` groups them, each group in pair.txt order, and numbered through the groups.  ``level``,
    ``level_lambda``: the seam levelling of :func:`texture_mesh`.  -> the info of :func:`texture_mesh`."""
    check_texture_args(scale, max_cell, max_size, min_px, "texture_scan", level, level_lambda)
    dev = torch.device(device)
    mesh = load_mesh(mesh_ply, dev)
    scan = ScanFolder(scan_out_folder)
    vids = [ref for ref, _ in read_pair_file(os.path.join(pair_folder, "pair.txt"))]
    groups = scan.groups(vids, scan.image_size).values()              # views by image size, each in pair.txt order
    images = [torch.from_numpy(np.stack([scan.image(i) for i in ids])).to(dev) for ids in groups]
    cam_t = [torch.from_numpy(np.stack([scan.cam(i) for i in ids])) for ids in groups]
    out, info = texture_mesh(mesh, images, cam_t, scale=scale, max_cell=max_cell, max_size=max_size, min_px=min_px, chunk=chunk,
                             level=level, level_lambda=level_lambda)
    if info["H"] == 0:
        raise ValueError(f"texture_scan: {scan_out_folder}: a mesh of {info['faces']} faces and {info['views']} views: nothing to texture")
    write_textured_obj(prefix, mesh, out)
    print(f"{os.path.basename(prefix)}.obj: {format_texture(info)}", flush=True)
    return info


# ---------------------------------------------------------------------------------------------------------------------- CLI
def add_texture_args(ap: argparse.ArgumentParser) -> None:
    """The options of DESIGN §1.17 that ``infer --texture`` shares."""
    ap.add_argument("--texture_scale", type=float, default=None, metavar="S",
                    help=f"texture: texels per image pixel along a face's longest edge (default {DEFAULTS['scale']})")
    ap.add_argument("--texture_max_cell", type=int, default=None, metavar="C",
                    help=f"texture: the largest cell of a face, a power of two in 4..{MAX_CELL} (default {DEFAULTS['max_cell']})")
    ap.add_argument("--texture_max_size", type=int, default=None, metavar="N",
                    help=f"texture: the widest atlas, in texels, at most {MAX_SIZE} (default {DEFAULTS['max_size']})")
    ap.add_argument("--texture_min_px", type=int, default=None, metavar="P",
                    help=f"texture: pixels a face needs in its best view to take its colour from it (default {DEFAULTS['min_px']})")
    ap.add_argument("--texture_level", type=int, default=None, metavar="ITER",
                    help="texture: level the seams between faces coloured from different views: per-view offsets and ITER "
                         f"iterations of per-vertex corrections (DESIGN §1.19; default {DEFAULTS['level']}: no levelling)")
    ap.add_argument("--texture_level_lambda", type=float, default=None, metavar="L",
                    help=f"--texture_level: the weight of the corrections' smoothness over a face (default {DEFAULTS['level_lambda']})")


def texture_kwargs(ap: argparse.ArgumentParser, args, enabled: bool = True) -> Dict[str, object]:
    """The --texture_* options -> the keywords of :func:`texture_scan`.  ap.error for one given without --texture (``enabled``
    false), for a value outside its range and for --texture_level_lambda without --texture_level."""
    given = {k: getattr(args, "texture_" + k) for k in DEFAULTS}
    if not enabled:
        names = [f"--texture_{k}" for k, val in given.items() if val is not None]
        if names:
            ap.error(f"{', '.join(names)} belong to --texture")
        return {}
    if given["level_lambda"] is not None and not given["level"]:
        ap.error("--texture_level_lambda belongs to --texture_level ITER with ITER >= 1")
    kw = {k: DEFAULTS[k] if val is None else val for k, val in given.items()}
    try:
        check_texture_args(kw["scale"], kw["max_cell"], kw["max_size"], kw["min_px"], "--texture", kw["level"], kw["level_lambda"])
    except ValueError as e:
        ap.error(str(e))
    if given["level"] is None:                                        # without the option the keywords are what they were
        del kw["level"], kw["level_lambda"]
    return kw


def main(argv=None) -> Dict[str, Dict[str, object]]:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--testpath", required=True, help="the scenes: <testpath>/<scan>/pair.txt")
    ap.add_argument("--outdir", required=True, help="the infer output folder: <outdir>/<scan>/{cams,images}")
    ap.add_argument("--testlist", required=True, help="text file with one scan name per line")
    ap.add_argument("--mesh", default=None, help="the mesh file; {scan} is replaced (default <outdir>/{scan}_mesh.ply)")
    ap.add_argument("--device", default="cuda")
    add_texture_args(ap)
    args = ap.parse_args(argv)
    kw = texture_kwargs(ap, args)
    scans = read_testlist(args.testlist)
    out = {}
    for scan in scans:
        ply = (args.mesh or os.path.join(args.outdir, "{scan}_mesh.ply")).format(scan=scan)
        out[scan] = texture_scan(os.path.join(args.outdir, scan), ply, os.path.join(args.testpath, scan),
                                 os.path.join(args.outdir, f"{scan}_textured"), device=args.device, **kw)
    return out


if __name__ == "__main__":
    main()
