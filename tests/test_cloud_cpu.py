"""Fused clouds with normals and voxel merging, the parts that need no GPU: the restated normal rule is exact on
planes, the PLY writer and readers, the command lines, the C header."""
import os
import re

import numpy as np
import pytest

import cloud_ref as C
from cds_mvsnet_amd import _lib, fusion, gipuma, infer, pointcloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLANE_F64_DEG = 1e-5      # measured 8.5e-7 deg from float64 depths on the 24x40 image at depth ~650
PLANE_F32_DEG = 5e-3      # measured 4.8e-4 deg from float32 depths (2^-24 relative depth error over a 5-pixel baseline)


@pytest.mark.parametrize("dtype,bound", [(np.float64, PLANE_F64_DEG), (np.float32, PLANE_F32_DEG)], ids=["f64", "f32"])
def test_plane_exactness(dtype, bound):
    depth, K, E, true_n = C.tilted_plane(24, 40, dtype)
    assert 600 < depth.min() and depth.max() < 700
    normals, ok = C.depth_normals(depth, K, E, radius=2, jump=0.01, min_pts=6)
    assert ok.all()                                                   # also the border pixels: 9 of 25 neighbours are enough
    err = C.angle_deg(normals, ok, true_n)
    print(f"{np.dtype(dtype).name} depths: max angle {err:.2e} deg")
    assert err < bound
    assert np.abs(np.linalg.norm(normals, axis=0) - 1).max() < 1e-12


def test_restatement_decisions():
    """Invalid centres, too few neighbours, and a depth step that the jump test must not bridge."""
    depth, K, E, true_n = C.tilted_plane(9, 12, np.float32, f=48.0)
    depth[:, 6:] *= 1.05                                              # a 5 % step between columns 5 and 6
    depth[2, 2], depth[3, 9], depth[0, 0] = 0.0, np.nan, np.inf
    valid = np.ones(depth.shape, np.uint8)
    valid[7, :] = 0
    normals, ok = C.depth_normals(depth, K, E, valid=valid, radius=1, jump=0.01, min_pts=6)
    assert not ok[2, 2] and not ok[3, 9] and not ok[0, 0] and not ok[7].any()
    assert not ok[8].any()                                            # row 8: only its own three pixels per window
    assert not ok[0, 11] and ok[4, 4] and ok[4, 5] and ok[4, 6]       # a corner has 4 pixels; the step's sides fit alone
    assert (normals[:, ok == 0] == 0).all()
    # both sides of the step are pieces of planes through the camera's rays: scaling a plane's depths keeps its normal
    assert C.angle_deg(normals, ok, true_n) < PLANE_F32_DEG


def _cloud(n, seed=0):
    rs = np.random.RandomState(seed)
    pts = rs.randn(n, 3).astype(np.float32)
    col = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    nrm = rs.randn(n, 3)
    return pts, col, (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)


def test_ply_roundtrip_with_normals(tmp_path):
    pts, col, nrm = _cloud(37)
    path = str(tmp_path / "n.ply")
    fusion.write_ply(path, pts, col, nrm)
    head = open(path, "rb").read().split(b"end_header\n")[0].decode("ascii")
    assert re.findall(r"property (\w+) (\w+)", head) == [("float", "x"), ("float", "y"), ("float", "z"), ("float", "nx"),
                                                         ("float", "ny"), ("float", "nz"), ("uchar", "red"),
                                                         ("uchar", "green"), ("uchar", "blue")]
    assert os.path.getsize(path) == len(head) + len("end_header\n") + 37 * 27
    p, c, n = fusion.read_ply_full(path)
    assert np.array_equal(p, pts) and np.array_equal(c, col) and np.array_equal(n, nrm)
    assert p.dtype == np.float32 and c.dtype == np.uint8 and n.dtype == np.float32
    assert np.array_equal(pointcloud.read_ply_points(path), pts)      # what dtu_eval / tt_eval read: x, y, z by name
    with pytest.raises(ValueError):
        fusion.write_ply(path, pts, col, nrm[:5])


def test_ply_without_normals_is_unchanged(tmp_path):
    pts, col, _ = _cloud(5, seed=1)
    path = str(tmp_path / "p.ply")
    fusion.write_ply(path, pts, col)
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n"
              b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    body = b"".join(pts[i].astype("<f4").tobytes() + col[i].tobytes() for i in range(5))
    assert open(path, "rb").read() == header + body
    p, c = fusion.read_ply(path)
    assert np.array_equal(p, pts) and np.array_equal(c, col)
    p, c, n = fusion.read_ply_full(path)
    assert np.array_equal(p, pts) and np.array_equal(c, col) and n is None
    fusion.write_ply(path, pts[:0], col[:0], np.zeros((0, 3), np.float32))            # an empty cloud with normals
    p, c, n = fusion.read_ply_full(path)
    assert p.shape == (0, 3) and c.shape == (0, 3) and n.shape == (0, 3)


_IO = ["--testpath", "a", "--outdir", "b", "--testlist", "c"]


def test_cli_flags(capsys):
    for mod in (fusion, infer):
        a = mod.parse_args(_IO)
        assert (a.normals, a.normal_radius, a.normal_jump, a.normal_min_pts, a.merge_voxel, a.merge_min_points) == \
            (False, 2, 0.01, 6, None, 1)
        a = mod.parse_args(_IO + ["--normals", "--normal_radius", "3", "--normal_jump", "0.02", "--normal_min_pts", "9",
                                  "--merge_voxel", "0.5", "--merge_min_points", "2", "--filter_method", "dynamic"])
        assert (a.normals, a.normal_radius, a.normal_jump, a.normal_min_pts, a.merge_voxel, a.merge_min_points) == \
            (True, 3, 0.02, 9, 0.5, 2)
        assert fusion.cloud_kwargs(a) == dict(normals=True, normal_radius=3, normal_jump=0.02, normal_min_pts=9, merge_voxel=0.5,
                                              merge_min_points=2)
    a = infer.parse_args(_IO + ["--filter_method", "gipuma", "--merge_voxel", "2", "--merge_min_points", "3"])
    assert (a.merge_voxel, a.merge_min_points, a.normals) == (2.0, 3, False)
    a = gipuma.parse_args(["--outdir", "b", "--testlist", "c", "--merge_voxel", "2", "--merge_min_points", "3"])
    assert (a.merge_voxel, a.merge_min_points) == (2.0, 3)
    assert gipuma.parse_args(["--outdir", "b", "--testlist", "c"]).merge_voxel is None
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        infer.parse_args(_IO + ["--filter_method", "gipuma", "--normals"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--normals" in err and "not implemented" in err
    with pytest.raises(SystemExit):                                   # gipuma's own command line has no --normals
        gipuma.parse_args(["--outdir", "b", "--testlist", "c", "--normals"])
    assert fusion.format_cloud({"points": 3}) == ""
    assert fusion.format_cloud({"no_normal": 0.0123, "merged_from": 99}) == ", no normal 1.2%, merged from 99"


def test_header_declares_the_cloud_symbols():
    header = open(os.path.join(ROOT, "include", "cds_mvsnet_hip.h")).read()
    protos = dict(re.findall(r"^int\s+(cds_\w+)\s*\(([^;]*?)\);", header, re.M | re.S))
    for name, nargs in (("cds_depth_normals_f32", 11), ("cds_voxel_merge_f32", 12)):
        assert name in protos, name
        assert len(protos[name].split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert "cloud.hip" in open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "Makefile")).read()


def test_restated_merge():
    """The per-voxel loop on a case small enough to check by hand."""
    pts = np.array([[0.1, 0.1, 0.1], [5.0, 5.0, 5.0], [0.3, 0.2, 0.1], [0.2, 0.3, 0.4]], np.float32)
    col = np.array([[0, 10, 255], [7, 8, 9], [1, 11, 255], [1, 10, 254]], np.uint8)
    nrm = np.array([[0, 0, 1], [1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    m = C.merge_voxels(pts, col, 1.0, nrm)
    assert m["counts"].tolist() == [3, 1]
    assert np.array_equal(m["points"][0], (pts[[0, 2, 3]].astype(np.float64).sum(0) / 3).astype(np.float32))
    assert m["colors"].tolist() == [[1, 10, 255], [7, 8, 9]]          # 2/3 -> 1, 31/3 -> 10, 764/3 = 254.67 -> 255
    assert np.allclose(m["normals"], [[0, 1, 0], [1, 0, 0]])          # the opposing pair cancels
    assert C.merge_voxels(pts, col, 1.0, nrm, min_points=2)["counts"].tolist() == [3]
    z = C.merge_voxels(pts[[0, 2]], col[[0, 2]], 1.0, nrm[[0, 2]])
    assert z["normals"].tolist() == [[0, 0, 0]]                       # a zero sum stays zero
