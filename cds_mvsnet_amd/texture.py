"""A mesh textured from the images of its scan, on the GPU: a texture atlas and an OBJ that Blender or MeshLab opens (DESIGN §1.17;
the rule is in include/cds_mvsnet_hip.h).

Every face takes its colour from one view, the one in which the rasteriser of §1.10 shows most of it, and owns one square cell of
the atlas, sized from its longest edge in that view.  The cells are packed along a Z-order curve, every texel of a cell is the
bilinear sample of the view's image at the projection of its surface point, and faces that no view sees keep their interpolated
vertex colours.  The output is a function of the input alone.  The hot paths are the kernels of ``csrc/mesh_texture.hip``
(``cds_texture_votes``, ``cds_texture_best``, ``cds_texture_cells``, ``cds_texture_place``, ``cds_texture_fill``) behind
``render.render_mesh``; torch sorts the cell sizes and sums the units between two launches.  There is no CPU path.

    python -m cds_mvsnet_amd.texture --testpath <scenes> --outdir <out> --testlist <list> [--mesh "<out>/{scan}_mesh.ply"]
        [--texture_scale S] [--texture_max_cell C] [--texture_max_size N] [--texture_min_px P]

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
DEFAULTS = dict(scale=1.0, max_cell=256, max_size=16384, min_px=1)
VOTE_RUNS = 1                  # cds_texture_votes: one add per run of equal faces (profiles/mesh_texture.md)
FILL_PER_UNIT = 1              # cds_texture_fill: one thread per 4 x 4 unit, one search for its 16 texels (profiles/mesh_texture.md)


def _is_pow2(n: int) -> bool:
    return n >= 1 and n & (n - 1) == 0


def check_texture_args(scale, max_cell, max_size, min_px, what: str = "texture_mesh") -> Tuple[float, int, int, int]:
    """-> (scale, max_cell, max_size, min_px); ValueError unless scale is finite and > 0, max_cell a power of two in 4..4096,
    max_size in 4..32768 and min_px >= 1."""
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


def texture_mesh(mesh_dict: Dict[str, Tensor], images, cams, scale: float = 1.0, max_cell: int = 256, max_size: int = 16384,
                 min_px: int = 1, chunk: int = 8):
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
    neither launches anything."""
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
    tab = torch.cat([camera_table(cam) for _, cam in groups]) if groups else torch.zeros((0, CAM_DOUBLES), dtype=torch.float64)
    dev = check_mesh_device(vert, col, faces, what)
    for img, _ in groups:
        if not img.is_cuda or img.device != dev:
            raise RuntimeError(f"{what}: images must be on {dev}; there is no CPU fallback")
    v = int(tab.shape[0])
    out = {"atlas": torch.zeros((0, 0, 3), dtype=torch.uint8, device=dev), "uv": torch.zeros((nf, 3, 2), dtype=torch.int32, device=dev),
           "view": torch.full((nf,), -1, dtype=torch.int32, device=dev), "cell": torch.zeros((nf, 3), dtype=torch.int32, device=dev)}
    info = {"H": 0, "W": 0, "faces": nf, "unseen": nf, "units": (0, 0), "views": v}
    if nf == 0 or v == 0:
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
        total, unseen = (int(x) for x in torch.stack([ends[-1], (out["view"] < 0).sum()]).cpu())   # the one read
        ah, aw = atlas_size(total, max_size, what)
        starts = ends - units
        check(lib.cds_texture_place(order.data_ptr(), starts.data_ptr(), nf, total, max_cell, out["cell"].data_ptr(),
                                    out["uv"].data_ptr(), stream), "cds_texture_place")
        out["atlas"] = torch.empty((ah, aw, 3), dtype=torch.uint8, device=dev)
        check(lib.cds_texture_fill(vert.data_ptr(), col.data_ptr(), nv, faces.data_ptr(), nf, tab.data_ptr(), pixels.data_ptr(),
                                   int(pixels.numel()), views.data_ptr(), v, out["view"].data_ptr(), out["cell"].data_ptr(),
                                   order.data_ptr(), starts.data_ptr(), total, max_cell, ah, aw, out["atlas"].data_ptr(), FILL_PER_UNIT,
                                   stream), "cds_texture_fill")
    info.update(H=ah, W=aw, unseen=unseen, units=(total, (ah // 4) * (aw // 4)))
    return out, info


def format_texture(info: Dict[str, object]) -> str:
    used, room = info["units"]
    return (f"atlas {info['W']} x {info['H']}, {100.0 * used / room if room else 0.0:.1f} % of its units used, {info['faces']} faces from "
            f"{info['views']} views, {100.0 * info['unseen'] / info['faces'] if info['faces'] else 0.0:.2f} % unseen")


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
                 max_size: int = 16384, min_px: int = 1, device: str = "cuda", chunk: int = 8) -> Dict[str, object]:
    """Texture a mesh from the views of ``<pair_folder>/pair.txt``, in that order: the images ``<scan_out_folder>/images/%08d.jpg``
    with the cameras of ``<scan_out_folder>/cams/%08d_cam.txt``, and write ``<prefix>.{obj,mtl,png}``.  ``mesh_ply``: a file of
    ``mesh.write_mesh_ply``, or the mesh dict of the mesh stage on the device.  The views are grouped by image size as
    ``render.render_scan`` groups them, each group in pair.txt order, and numbered through the groups.  -> the info of
    :func:`texture_mesh`."""
    check_texture_args(scale, max_cell, max_size, min_px, "texture_scan")
    dev = torch.device(device)
    mesh = load_mesh(mesh_ply, dev)
    scan = ScanFolder(scan_out_folder)
    vids = [ref for ref, _ in read_pair_file(os.path.join(pair_folder, "pair.txt"))]
    groups = scan.groups(vids, scan.image_size).values()              # views by image size, each in pair.txt order
    images = [torch.from_numpy(np.stack([scan.image(i) for i in ids])).to(dev) for ids in groups]
    cam_t = [torch.from_numpy(np.stack([scan.cam(i) for i in ids])) for ids in groups]
    out, info = texture_mesh(mesh, images, cam_t, scale=scale, max_cell=max_cell, max_size=max_size, min_px=min_px, chunk=chunk)
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


def texture_kwargs(ap: argparse.ArgumentParser, args, enabled: bool = True) -> Dict[str, object]:
    """The --texture_* options -> the keywords of :func:`texture_scan`.  ap.error for one given without --texture (``enabled``
    false) and for a value outside its range."""
    given = {k: getattr(args, "texture_" + k) for k in DEFAULTS}
    if not enabled:
        names = [f"--texture_{k}" for k, val in given.items() if val is not None]
        if names:
            ap.error(f"{', '.join(names)} belong to --texture")
        return {}
    kw = {k: DEFAULTS[k] if val is None else val for k, val in given.items()}
    try:
        check_texture_args(kw["scale"], kw["max_cell"], kw["max_size"], kw["min_px"], "--texture")
    except ValueError as e:
        ap.error(str(e))
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
