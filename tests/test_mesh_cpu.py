"""The meshing rule of DESIGN §1.9 as restated in mesh_ref.py, checked on volumes whose surface is known, and the parts of
cds_mvsnet_amd.mesh that need no device: the PLY files and the argument checks."""
import os

import numpy as np
import pytest

import mesh_ref as M
from cds_mvsnet_amd import infer, mesh, pointcloud


def _closed(m, what):
    tp = M.topology(m["faces"], len(m["vertices"]))
    assert tp["used_vertices"] == len(m["vertices"]), f"{what}: vertices that no face uses"
    assert (tp["edge_uses"] == 2).all(), f"{what}: an edge that is not in exactly 2 triangles"
    assert tp["directed_unique"] and tp["reverse_present"], f"{what}: inconsistent winding"
    assert tp["euler"] == 2, f"{what}: V - E + F = {tp['euler']}"
    return tp


def test_analytic_sphere():
    """|X - c| - r with c = (9.3, 9.7, 9.1), r = 6.37 on 24^3 lattice points in 3 blocks per axis.  Measured with the
    restatement: 2286 vertices, 4568 faces, volume 0.98767 of the sphere's, vertices within 0.05901 voxel of the sphere (the
    distance field is linear along an edge only to second order).  The geometric bounds are those numbers plus 25 %."""
    vol, m = M.analytic_case("sphere")
    assert len(vol["keys"]) == 27
    _closed(m, "sphere")
    assert (len(m["vertices"]), len(m["faces"])) == (2286, 4568)
    c, r = np.array(M.ANALYTIC["sphere"]["centre"]), M.ANALYTIC["sphere"]["radius"]
    ratio = M.signed_volume(m["vertices"], m["faces"]) / (4.0 / 3.0 * np.pi * r ** 3)
    dist = np.abs(np.linalg.norm(m["vertices"].astype(np.float64) - c, axis=1) - r).max()
    print(f"volume ratio {ratio:.5f}, largest distance {dist:.5f} voxel")
    assert ratio > 0 and abs(1.0 - ratio) <= 1.25 * (1.0 - 0.98767)
    assert dist <= 1.25 * 0.05901
    # the faces cross block borders, and the order is (block key, local cube index, tetrahedron, triangle)
    blocks = np.unique((m["cubes"] // 8) @ np.array([1, 3, 9]))
    assert len(blocks) > 8
    key = ((m["cubes"] // 8) @ np.array([1, 3, 9])) * 512 + (m["cubes"] % 8) @ np.array([1, 8, 64])
    assert (np.diff(key) >= 0).all()


def test_lattice_aligned_centre():
    """Centre (9, 10, 9) and r = 6: 30 lattice points have sum == 0.  They are outside, the vertices of their edges coincide with
    them and 300 triangles have no area; they are kept and the surface stays closed."""
    vol, m = M.analytic_case("aligned")
    assert int((vol["sum"] == 0).sum()) == 30
    _closed(m, "aligned")
    assert M.degenerate_faces(m["vertices"], m["faces"]) == 300
    assert M.signed_volume(m["vertices"], m["faces"]) > 0


def test_removed_block():
    """Without block (1, 1, 0) the mesh has a boundary, no edge has more than two triangles, and no triangle comes from a cube
    with a corner in the missing block."""
    vol, m = M.analytic_case("hole")
    full = M.analytic_case("sphere")[1]
    assert len(vol["keys"]) == 26 and 0 < len(m["faces"]) < len(full["faces"])
    tp = M.topology(m["faces"], len(m["vertices"]))
    assert (tp["edge_uses"] == 1).any() and tp["edge_uses"].max() == 2
    assert tp["directed_unique"]
    corners = m["cubes"][:, None, :] + np.array([[o & 1, (o >> 1) & 1, o >> 2] for o in range(8)])[None]
    b = corners // 8
    missing = (b[..., 0] == 1) & (b[..., 1] == 1) & (b[..., 2] == 0)
    assert not missing.any() and (b >= 0).all() and (b < 3).all()
    # the same holds with a weight threshold: points seen once are as good as missing
    vol2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in M.analytic_case("sphere")[0].items()}
    vol2["n"][4] = 1                                              # block (1, 1, 0) has key 4
    m2 = M.extract(vol2, 2)
    assert np.array_equal(m2["faces"], m["faces"]) and np.array_equal(m2["vertices"], m["vertices"])


def test_sphere_scene_restatement():
    """26 cameras on the directions {-1,0,1}^3 \\ 0 at 4 r around a sphere of r = 9 voxels, 48 x 48 analytic depth maps, T = 2.5
    voxels, min_weight 2.  Measured with the restatement: 120 blocks in a 5^3 grid, 4630 vertices, 9256 faces, closed with Euler
    characteristic 2, volume 1.01630 of the sphere's, vertices within 0.40666 voxel of the sphere (nearest-pixel depth near the
    silhouettes).  Bounds: those numbers plus 25 %."""
    sc, vol, m = M.sphere_case()
    assert vol["nb"].tolist() == [5, 5, 5] and len(vol["keys"]) == 120
    _closed(m, "sphere scene")
    assert (len(m["vertices"]), len(m["faces"])) == (4630, 9256)
    r, s = sc["radius"], sc["voxel"]
    ratio = M.signed_volume(m["vertices"].astype(np.float64) - sc["centre"], m["faces"]) / (4.0 / 3.0 * np.pi * r ** 3)
    dist = (np.abs(np.linalg.norm(m["vertices"].astype(np.float64) - sc["centre"], axis=1) - r) / s).max()
    print(f"volume ratio {ratio:.5f}, largest distance {dist:.5f} voxel")
    assert abs(ratio - 1.0) <= 1.25 * 0.01630 and dist <= 1.25 * 0.40666
    assert int((vol["nc"] > 0).sum()) > 0 and len(np.unique(m["colors"], axis=0)) > 10


def test_allocation_is_points_and_neighbours():
    pts = np.array([[0.1, 0.1, 0.1], [0.2, 0.3, 0.1], [9.0, 0.1, 0.1]], np.float32)
    vol = M.allocate(pts, 0.25, 1.0)                              # blocks of side 2: the points lie in x blocks 1 and 5
    assert vol["origin"].tolist() == [-2.0, -2.0, -2.0] and vol["nb"].tolist() == [7, 3, 3]
    bx = vol["keys"] % 7
    assert len(vol["keys"]) == 6 * 9 and sorted(set(bx.tolist())) == [0, 1, 2, 4, 5, 6]


# ------------------------------------------------------------------------------------------------------------------- files
def test_ply_round_trip(tmp_path):
    _, m = M.analytic_case("sphere")
    path = str(tmp_path / "m.ply")
    mesh.write_mesh_ply(path, m["vertices"], m["colors"], m["faces"])
    v, c, f = mesh.read_mesh_ply(path)
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32
    assert np.array_equal(v, m["vertices"]) and np.array_equal(c, m["colors"]) and np.array_equal(f, m["faces"])
    head = open(path, "rb").read(400).decode("ascii", "replace")
    assert "format binary_little_endian 1.0" in head and "property list uchar int vertex_indices" in head
    assert os.path.getsize(path) == head.index("end_header\n") + 11 + 15 * len(v) + 13 * len(f)
    # the evaluations read its vertices
    assert np.array_equal(pointcloud.read_ply_points(path), m["vertices"])
    first = open(path, "rb").read()
    mesh.write_mesh_ply(path, m["vertices"], m["colors"], m["faces"])
    assert open(path, "rb").read() == first


def test_empty_mesh_file(tmp_path):
    path = str(tmp_path / "e.ply")
    mesh.write_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32))
    v, c, f = mesh.read_mesh_ply(path)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    assert pointcloud.read_ply_points(path).shape == (0, 3)
    assert b"element vertex 0\n" in open(path, "rb").read() and b"element face 0\n" in open(path, "rb").read()


def test_file_argument_checks(tmp_path):
    v, c = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.uint8)
    with pytest.raises(ValueError):
        mesh.write_mesh_ply(str(tmp_path / "a.ply"), v, c, np.array([[0, 1, 3]], np.int32))        # index outside the vertices
    with pytest.raises(ValueError):
        mesh.write_mesh_ply(str(tmp_path / "a.ply"), v, c[:2], np.array([[0, 1, 2]], np.int32))
    with pytest.raises(ValueError):
        mesh.write_mesh_ply(str(tmp_path / "a.ply"), v, c, np.array([[0, 1, 2, 0]], np.int32))
    with open(tmp_path / "b.ply", "wb") as f:
        f.write(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        mesh.read_mesh_ply(str(tmp_path / "b.ply"))
    path = str(tmp_path / "t.ply")
    mesh.write_mesh_ply(path, v, c, np.array([[0, 1, 2]], np.int32))
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:-4])
    with pytest.raises(ValueError):
        mesh.read_mesh_ply(path)


# --------------------------------------------------------------------------------------------------------------- arguments
def test_voxel_and_trunc_checks():
    assert mesh.check_voxel(0.5) == (0.5, 2.0)
    assert mesh.check_voxel(0.5, 0.5) == (0.5, 0.5) and mesh.check_voxel(0.5, 4.0) == (0.5, 4.0)
    for voxel in (0.0, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="voxel must be positive"):
            mesh.check_voxel(voxel)
    for trunc in (0.49, 4.01, float("nan"), -1.0):
        with pytest.raises(ValueError, match="trunc must lie in"):
            mesh.check_voxel(0.5, trunc)
    mesh.check_grid([512, 512, 256], 1.0)                         # exactly the cap
    with pytest.raises(ValueError, match="raise --mesh_voxel"):
        mesh.check_grid([512, 512, 257], 1.0)


def test_scan_argument_checks(tmp_path):
    """What is refused before any file is read or any device touched."""
    with pytest.raises(ValueError, match="gipuma"):
        mesh.mesh_scan(str(tmp_path), str(tmp_path), str(tmp_path / "m.ply"), 1.0, method="gipuma")
    with pytest.raises(ValueError, match="voxel must be positive"):
        mesh.mesh_scan(str(tmp_path), str(tmp_path), str(tmp_path / "m.ply"), 0.0)
    with pytest.raises(ValueError, match="trunc must lie in"):
        mesh.mesh_scan(str(tmp_path), str(tmp_path), str(tmp_path / "m.ply"), 1.0, trunc=9.0)
    with pytest.raises(ValueError, match="min_weight"):
        mesh.mesh_scan(str(tmp_path), str(tmp_path), str(tmp_path / "m.ply"), 1.0, min_weight=0)
    assert not (tmp_path / "m.ply").exists()


def test_command_lines_refuse_gipuma(tmp_path, capsys):
    base = ["--testpath", str(tmp_path), "--outdir", str(tmp_path), "--testlist", str(tmp_path / "l.txt")]
    with pytest.raises(SystemExit):
        mesh.main(base + ["--mesh_voxel", "1.0", "--filter_method", "gipuma"])
    assert "gipuma" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mesh.main(base)                                            # --mesh_voxel is required here
    capsys.readouterr()
    with pytest.raises(SystemExit):
        infer.parse_args(base + ["--fuse", "--filter_method", "gipuma", "--mesh_voxel", "1.0"])
    assert "--mesh_voxel is not implemented for --filter_method gipuma" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        infer.parse_args(base + ["--fuse", "--mesh_voxel", "1.0", "--mesh_trunc", "9.0"])
    assert "trunc must lie in" in capsys.readouterr().err
    args = infer.parse_args(base + ["--fuse", "--mesh_voxel", "2.0"])
    assert args.mesh_voxel == 2.0 and args.mesh_trunc is None and args.mesh_min_weight == 2
    assert infer.parse_args(base + ["--fuse"]).mesh_voxel is None
