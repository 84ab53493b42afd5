"""The numpy restatement of the simplification rule (mesh_simplify_ref.py) against things known by construction:
counts and volumes of the analytic sphere, a cube whose corners and edges the quadric keeps and the mean rounds off, a plane, a
two-sided plate, a cone whose tangent planes meet in its apex; and the parts of the public interface that need no GPU: argument
checks, the header, the binding and the Makefile, the command-line options and the printed line."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_ref as M
import mesh_simplify_ref as R
from cds_mvsnet_amd import _lib, infer, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sphere():
    m = M.analytic_case("sphere")[1]
    return m["vertices"], m["colors"], m["faces"]


def _identity(t):
    r = t.index(min(t))
    return t[r], t[(r + 1) % 3], t[(r + 2) % 3]


def _valid(out, info):
    v, c, f = out["vertices"], out["colors"], out["faces"]
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32
    assert v.shape == (info["vertices"][1], 3) == c.shape and f.shape == (info["faces"][1], 3)
    assert info["faces"][0] == info["faces"][1] + info["collapsed"] + info["duplicates"]
    if len(f):
        assert f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)          # dense: every vertex is used
        assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
        ids = [_identity(t) for t in f.tolist()]
        assert len(set(ids)) == len(ids)                                                       # no face twice
    assert np.isfinite(v).all()


# ------------------------------------------------------------------------------------------------------------ the sphere
@pytest.mark.parametrize("cell, nv, nf, collapsed, duplicates, vol_mean, vol_quadric",
                         [(1.0, 562, 1136, 3428, 4, 1055.05, 1062.88), (2.0, 163, 330, 4236, 2, 996.9, 1042.6)])
def test_sphere_counts_and_volumes(cell, nv, nf, collapsed, duplicates, vol_mean, vol_quadric):
    v, c, f = _sphere()
    assert v.shape == (2286, 3) and f.shape == (4568, 3) and abs(M.signed_volume(v, f) - 1069.34) < 0.01 and R.closed(f)
    vols = {}
    for placement in ("mean", "quadric"):
        out, info, detail = R.simplify(v, c, f, cell, placement)
        _valid(out, info)
        assert info == {"vertices": (2286, nv), "faces": (4568, nf), "clusters": nv, "collapsed": collapsed,
                        "duplicates": duplicates, "fallback": 0}
        assert R.closed(out["faces"])
        vols[placement] = M.signed_volume(out["vertices"], out["faces"])
    print(f"cell {cell}: volume {vols['mean']:.2f} (mean), {vols['quadric']:.2f} (quadric) of 1069.34")
    assert abs(vols["mean"] - vol_mean) < 0.06 and abs(vols["quadric"] - vol_quadric) < 0.06
    assert vols["mean"] < vols["quadric"] < 1069.34            # chords cut a convex body; the quadric vertex lies further out


def test_sphere_mean_is_the_voxel_mean_and_faces_do_not_depend_on_placement():
    import tt_eval_ref as T
    v, c, f = _sphere()
    a, ia, da = R.simplify(v, c, f, 1.0, "mean")
    b, ib, db = R.simplify(v, c, f, 1.0, "quadric")
    assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(a["colors"], b["colors"])
    means, keys, counts = T.voxel_down_sample(v, 1.0)          # the restatement cds_voxel_merge_f32 is held to
    assert np.array_equal(da["positions"].view(np.uint32), means.view(np.uint32)) and np.array_equal(keys, np.unique(R.cell_keys(v, 1.0)))
    assert (np.abs(db["positions"].astype(np.float64) - da["positions"]).max(1) <= 1.0).all()   # rule 4's last condition


def test_sphere_closed_at_every_cell_one_cluster_and_debris():
    v, c, f = _sphere()
    for cell in (0.25, 0.5, 1.5, 3.0):
        out, info, _ = R.simplify(v, c, f, cell)
        _valid(out, info)
        assert R.closed(out["faces"]) and info["fallback"] == 0, cell
    out, info, _ = R.simplify(v, c, f, 100.0)
    assert info == {"vertices": (2286, 0), "faces": (4568, 0), "clusters": 1, "collapsed": 4568, "duplicates": 0, "fallback": 0}
    _valid(out, info)
    vd, cd, fd = C.sphere_with_debris()
    out, info, detail = R.simplify(vd, cd, fd, 2.0)
    assert info["clusters"] == 167 and info["vertices"] == (2294, 163) and info["faces"] == (4576, 330)
    assert not detail["kept"][np.unique(detail["cluster"][2286:])].any()                        # the tetrahedra's clusters go
    sphere_only = R.simplify(v, c, f, 2.0)[0]
    assert np.array_equal(out["faces"], sphere_only["faces"])


# -------------------------------------------------------------------------------------------------------------- the cube
def test_cube_quadric_keeps_corners_and_edges():
    v, c, f = R.cube()
    assert v.shape == (1538, 3) and f.shape == (3072, 3) and R.closed(f) and abs(M.signed_volume(v, f) - 64.0) < 1e-4
    res = {}
    for placement in ("quadric", "mean"):
        out, info, _ = R.simplify(v, c, f, 1.0, placement)
        _valid(out, info)
        assert info["vertices"] == (1538, 98) and info["faces"] == (3072, 192) and info["fallback"] == 0 and R.closed(out["faces"])
        res[placement] = (M.signed_volume(out["vertices"], out["faces"]),) + R.cube_errors(out["vertices"])
        print(f"cube, {placement}: volume {res[placement][0]:.3f} of 64, corner to nearest vertex {res[placement][1]:.2e}, "
              f"from the surface {res[placement][2]:.2e}")
    q, m = res["quadric"], res["mean"]
    assert 63.9 < q[0] < 64.0 and m[0] < 60.0
    assert q[1] < 0.01 and m[1] > 0.2 and q[2] < 0.01 and m[2] > 0.1       # lam = tr / 1024 leaves about 1e-3 of the offset


# ----------------------------------------------------------------------------------------------------- plane, plate, cone
def test_tilted_plane_stays_a_plane():
    v, c, f, normal, origin = R.tilted_plane()
    ulp = float(np.spacing(np.float32(650.0)))
    assert np.abs((v.astype(np.float64) - origin) @ normal).max() <= ulp
    for placement in ("quadric", "mean"):
        out, info, _ = R.simplify(v, c, f, 1.0, placement)
        _valid(out, info)
        dist = np.abs((out["vertices"].astype(np.float64) - origin) @ normal).max()
        print(f"plane, {placement}: {info['vertices'][1]} vertices, {dist / ulp:.2f} ulp of 650 off the plane")
        assert info["vertices"][1] > 50 and dist <= ulp and info["fallback"] == 0


def test_plate_stays_two_sided():
    v, c, f = R.plate()
    out, info, detail = R.simplify(v, c, f, 1.0)
    _valid(out, info)
    ids = {_identity(t) for t in out["faces"].tolist()}
    assert info["duplicates"] == 0 and info["faces"][1] > 0 and info["faces"][1] % 2 == 0
    assert all(_identity(t[::-1]) in ids for t in out["faces"].tolist())
    n = len(v) // 2
    assert np.array_equal(detail["cluster"][:n], detail["cluster"][n:])                         # the sheets share their cells


def test_cone_apex_fallback_and_zero_area():
    v, c, f, apex, band = R.cone_band(0.6, 0.4)
    out, info, detail = R.simplify(v, c, f, 1.0)
    mean = R.simplify(v, c, f, 1.0, "mean")[2]
    k = detail["cluster"][band]
    assert (k == k[0]).all() and info["clusters"] == 2 and info["fallback"] == 0
    to_apex = np.linalg.norm(detail["positions"][k[0]].astype(np.float64) - apex)
    mean_to_apex = np.linalg.norm(mean["positions"][k[0]].astype(np.float64) - apex)
    print(f"cone, apex 0.6 cell away: the quadric vertex {to_apex:.4f} from the apex, the mean {mean_to_apex:.4f}")
    # every plane passes through the apex, so the unregularised minimum is the apex; lam = tr / 1024 leaves at most lam / (lam +
    # smallest eigenvalue) of the way: the eigenvalue along the axis is about sin^2(atan 0.4) = 0.14 tr, which gives 0.7 %
    assert to_apex < 0.02 and mean_to_apex > 0.55
    v, c, f, apex, band = R.cone_band(3.0, 0.1)
    out, info, detail = R.simplify(v, c, f, 1.0)
    mean = R.simplify(v, c, f, 1.0, "mean")[2]
    k = detail["cluster"][band]
    assert (k == k[0]).all() and info["fallback"] == 1 and detail["fallback"][k[0]]
    assert np.array_equal(detail["positions"][k[0]].view(np.uint32), mean["positions"][k[0]].view(np.uint32))
    assert not detail["fallback"][1 - k[0]]                                  # the far cluster, one plane: solved, next to its mean
    # zero area: three collinear vertices in one cell and one far vertex; both faces have a zero cross product
    vz = np.array([[5.0, 5.0, 5.0], [5.1, 5.1, 5.1], [5.2, 5.2, 5.2], [0.0, 0.0, 0.0]], np.float32)
    fz = np.array([[0, 1, 2], [3, 3, 0]], np.int32)
    out, info, detail = R.simplify(vz, R.colors_for(4, 1), fz, 1.0)
    assert info == {"vertices": (4, 0), "faces": (2, 0), "clusters": 2, "collapsed": 2, "duplicates": 0, "fallback": 2}
    assert np.array_equal(detail["positions"][1].view(np.uint32), (vz[:3].astype(np.float64).sum(0) / 3).astype(np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------ odd faces, unreferenced vertices
def test_repeated_indices_duplicates_windings_and_unreferenced_vertices():
    # six vertices in six cells of side 1, two more in no face (one in a cell of its own, one in the cell of vertex 0)
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2], [2, 2, 0], [2, 0, 2], [7, 7, 7], [0.1, 0.1, 0.1]], np.float32)
    f = np.array([[0, 1, 2], [1, 2, 0], [2, 1, 0], [0, 0, 3], [3, 4, 5], [0, 1, 2], [5, 3, 4], [0, 7, 1]], np.int32)
    col = R.colors_for(8, 2)
    out, info, detail = R.simplify(v, col, f, 1.0)
    _valid(out, info)
    assert info["clusters"] == 7 and detail["cluster"][0] == detail["cluster"][7]
    assert detail["collapsed"].tolist() == [False, False, False, True, False, False, False, True]
    assert detail["face_keep"].tolist() == [True, False, True, False, True, False, False, False]    # the lowest index of each identity
    assert info == {"vertices": (8, 6), "faces": (8, 3), "clusters": 7, "collapsed": 2, "duplicates": 3, "fallback": info["fallback"]}
    k = detail["cluster"]
    new = np.cumsum(detail["kept"]) - 1
    assert out["faces"].tolist() == [new[k[[0, 1, 2]]].tolist(), new[k[[2, 1, 0]]].tolist(), new[k[[3, 4, 5]]].tolist()]   # corners as they stood
    assert not detail["kept"][k[6]]                                                                # the lone vertex's cluster goes
    # the colour of the cluster of vertices 0 and 7: (2 sum + k) / (2 k) per channel
    want = (2 * (col[0].astype(np.int64) + col[7]) + 2) // 4
    assert out["colors"][new[k[0]]].tolist() == want.tolist()
    # clusters come in ascending key order
    keys = np.unique(R.cell_keys(v, 1.0))
    assert np.array_equal(np.unique(R.cell_keys(v, 1.0), return_inverse=True)[1].reshape(-1), k) and (np.diff(keys) > 0).all()
    # empty inputs
    for vv, ff in ((v[:0], f[:0]), (v, f[:0])):
        out, info, _ = R.simplify(vv, col[:len(vv)], ff, 1.0)
        assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3) and info["clusters"] == 0


def test_random_faces_hold_the_invariants():
    rng = np.random.default_rng(4)
    v = rng.uniform(0, 6, (500, 3)).astype(np.float32)
    f = C.random_faces(500, 2000, seed=2)
    for placement in ("quadric", "mean"):
        out, info, detail = R.simplify(v, R.colors_for(500, 3), f, 1.5, placement)
        _valid(out, info)
        assert info["collapsed"] > 0 and info["duplicates"] > 0 and info["clusters"] > info["vertices"][1] - 1
        off = np.abs(detail["positions"].astype(np.float64) - R.simplify(v, R.colors_for(500, 3), f, 1.5, "mean")[2]["positions"])
        assert off.max() <= 1.5 + 1e-6


# ------------------------------------------------------------------------------------------------------- public interface
def test_no_cpu_path_and_argument_checks():
    v, col, f = (torch.from_numpy(a) for a in R.cube())
    m = {"vertices": v, "colors": col, "faces": f}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.simplify_mesh(m, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="cell must be positive"):
            mesh.simplify_mesh(m, bad)
    with pytest.raises(ValueError, match="placement"):
        mesh.simplify_mesh(m, 1.0, placement="median")
    with pytest.raises(ValueError, match="vertices must be"):
        mesh.simplify_mesh(dict(m, vertices=v.double()), 1.0)
    with pytest.raises(ValueError, match="colors must be"):
        mesh.simplify_mesh(dict(m, colors=col[:5]), 1.0)
    with pytest.raises(ValueError, match="cell must be positive"):
        mesh.mesh_scan("nowhere", "nowhere", "nowhere.ply", 1.0, simplify=-2.0)
    with pytest.raises(ValueError, match="placement"):
        mesh.mesh_scan("nowhere", "nowhere", "nowhere.ply", 1.0, simplify=2.0, placement="x")
    with pytest.raises(ValueError, match="cell must be positive"):
        mesh.clean_file("nowhere.ply", "nowhere.ply", simplify=float("nan"))
    assert mesh.PLACEMENTS == ("quadric", "mean")
    # the identities' first-of-a-run on the host, both ways of sorting
    ident = torch.tensor([[0, 1, 2], [0, 2, 1], [0, 1, 2], [1, 2, 3], [0, 2, 1], [1, 2, 3], [0, 1, 3]])
    assert mesh._first_of_identity(ident, 4).tolist() == [True, True, False, True, False, False, True]
    assert mesh._first_of_identity(ident, (1 << mesh.PACK_BITS) + 1).tolist() == [True, True, False, True, False, False, True]


def test_header_signatures_and_makefile():
    header = open(os.path.join(ROOT, "include", "cds_mvsnet_hip.h")).read()
    for name, nargs in (("cds_mesh_simplify_faces", 9), ("cds_mesh_simplify_quadric_f32", 13), ("cds_mesh_simplify_mark", 6),
                        ("cds_mesh_simplify_gather", 15)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\);", header, re.M | re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert "csrc/mesh_simplify.hip; DESIGN 1.12" in header
    makefile = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", makefile, re.M).group(1).split()
    assert "mesh_simplify.hip" in srcs and os.path.exists(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "mesh_simplify.hip"))
    source = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "mesh_simplify.hip")).read()
    assert "asm" not in source and "atomicAdd" not in source


def test_options_and_printed_line(capsys):
    ap = argparse.ArgumentParser()
    mesh.add_mesh_args(ap)
    args = ap.parse_args(["--mesh_voxel", "2"])
    assert args.mesh_simplify is None and args.mesh_simplify_placement == "quadric"
    args = ap.parse_args(["--mesh_voxel", "2", "--mesh_simplify", "8", "--mesh_simplify_placement", "mean"])
    assert (args.mesh_simplify, args.mesh_simplify_placement) == (8.0, "mean")
    base = ["--testpath", "x", "--testlist", "x", "--outdir", "x"]
    assert infer.parse_args(base + ["--fuse", "--mesh_voxel", "2", "--mesh_simplify", "4.5"]).mesh_simplify == 4.5
    assert infer.parse_args(base + ["--fuse", "--mesh_voxel", "2"]).mesh_simplify is None
    for extra in (["--mesh_simplify", "4"],                                                       # no mesh to simplify
                  ["--mesh_voxel", "2", "--mesh_simplify", "0"], ["--mesh_voxel", "2", "--mesh_simplify", "-1"],
                  ["--mesh_voxel", "2", "--mesh_simplify", "nan"], ["--mesh_voxel", "2", "--mesh_simplify", "inf"],
                  ["--mesh_voxel", "2", "--mesh_simplify", "4", "--mesh_simplify_placement", "median"]):
        with pytest.raises(SystemExit):
            infer.parse_args(base + ["--fuse"] + extra)
    for argv in (["--outdir", "x", "--testlist", "x", "--mesh_simplify", "4"],                      # neither --mesh_voxel nor --from_mesh
                 ["--outdir", "x", "--testlist", "x", "--from_mesh", "y", "--mesh_simplify", "0"],
                 ["--outdir", "x", "--testlist", "x", "--from_mesh", "y", "--mesh_simplify", "-3"]):
        with pytest.raises(SystemExit):
            mesh.main(argv)
    capsys.readouterr()
    old = {"vertices": 7, "faces": 5, "blocks": 3}
    assert mesh.format_mesh(old) == "7 vertices, 5 faces, 3 blocks"                                # the line of a run without the option
    info = {"vertices": (20, 7), "faces": (30, 5), "clusters": 9, "collapsed": 22, "duplicates": 3, "fallback": 1}
    line = mesh.format_mesh(dict(old, simplify=info))
    assert line.startswith("7 vertices, 5 faces, 3 blocks") and "simplified 20 -> 7 vertices and 30 -> 5 faces" in line
    assert "9 clusters, 22 faces collapsed, 3 duplicates, 1 fallbacks" in line
    both = mesh.format_mesh(dict(old, clean={"components": (4, 1), "vertices": (40, 20), "faces": (60, 30), "largest": 30, "rounds": 2},
                                 simplify=info))
    assert both.index("removed 3 of 4 components") < both.index("simplified 20 -> 7")
