"""The one PLY header parser / writer (cds_mvsnet_amd/ply.py) and the one reader of an ``infer`` scan folder
(mvs_io.ScanFolder, read_saved_cam, read_testlist).  CPU only; the files are a few hundred bytes."""
import os

import numpy as np
import pytest
import torch

from cds_mvsnet_amd import fusion, mesh, mvs_io, ply, pointcloud

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the fixed inputs of tests/golden/ply_*.ply, which the writers of the commit before ply.py produced from them
PTS = np.arange(15, dtype=np.float32).reshape(5, 3) * np.float32(0.25) - np.float32(1.0)
COL = ((np.arange(15).reshape(5, 3) * 17 + 3) % 256).astype(np.uint8)
NRM = np.roll(np.eye(3, dtype=np.float32), 1, 0)[np.arange(5) % 3] * np.float32(-1.0)
FACES = np.array([[0, 1, 2], [2, 3, 4], [0, 2, 4]], np.int32)

FACE_PROP = ("vertex_indices", ("u1", "i4"))
VERTEX = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("w", "f8")])


def _general_file(path, fmt):
    """edge (a list property) | vertex x y z w | face (a list property), with comment lines; -> the x y z written."""
    xyz = np.array([[0.5, -1.0, 2.0], [3.0, 4.5, -6.0]], np.float32)
    head = (f"ply\nformat {fmt} 1.0\ncomment made by a test\nobj_info nothing\nelement edge 1\nproperty list uchar int ends\n"
            "element vertex 2\nproperty float x\ncomment between\nproperty float32 y\nproperty float z\nproperty double w\n"
            "element face 1\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    with open(path, "wb") as f:
        f.write(head)
        if fmt == "ascii":
            f.write(b"2 0 1\n" + b"".join(("%r %r %r 7.0\n" % tuple(float(v) for v in r)).encode() for r in xyz) + b"3 0 1 1\n")
        else:
            end = "<" if fmt == "binary_little_endian" else ">"
            f.write(np.array([2], end + "u1").tobytes() + np.array([0, 1], end + "i4").tobytes())
            rec = np.zeros(2, VERTEX.newbyteorder(end))
            rec["x"], rec["y"], rec["z"], rec["w"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 7.0
            f.write(rec.tobytes())
            f.write(np.array([3], end + "u1").tobytes() + np.array([0, 1, 1], end + "i4").tobytes())
    return xyz


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_read_header_and_points(tmp_path, fmt):
    path = str(tmp_path / "g.ply")
    xyz = _general_file(path, fmt)
    with open(path, "rb") as f:
        got_fmt, elements = ply.read_header(f, path)
        assert f.read(1) != b""                                       # left at the data
    assert got_fmt == fmt
    assert [(name, count, list(props)) for name, count, props in elements] == [
        ("edge", 1, [("ends", ("u1", "i4"))]),
        ("vertex", 2, [("x", "f4"), ("y", "f4"), ("z", "f4"), ("w", "f8")]),
        ("face", 1, [FACE_PROP])]
    got = pointcloud.read_ply_points(path)
    assert got.dtype == np.float32 and np.array_equal(got, xyz)
    assert pointcloud.read_ply_points is ply.read_ply_points


def test_read_header_errors(tmp_path):
    def header(text):
        p = str(tmp_path / "h.ply")
        open(p, "wb").write(text)
        with open(p, "rb") as f:
            return ply.read_header(f, p)
    with pytest.raises(ValueError, match="not a PLY file"):
        header(b"plx\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ValueError, match="without end_header"):
        header(b"ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\n")
    with pytest.raises(ValueError, match="unknown PLY type half"):
        header(b"ply\nformat ascii 1.0\nelement vertex 0\nproperty half x\nend_header\n")
    with pytest.raises(ValueError, match="unknown PLY type half"):
        header(b"ply\nformat ascii 1.0\nelement face 0\nproperty list half int v\nend_header\n")
    with pytest.raises(ValueError, match="property before any element"):
        header(b"ply\nformat ascii 1.0\nproperty float x\nend_header\n")
    with pytest.raises(ValueError, match="unsupported PLY format binary_middle_endian"):
        header(b"ply\nformat binary_middle_endian 1.0\nend_header\n")


def test_writers_write_the_bytes_they_always_wrote(tmp_path):
    out = str(tmp_path / "o.ply")
    fusion.write_ply(out, PTS, COL)
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "ply_cloud.ply"), "rb").read()
    fusion.write_ply(out, PTS, COL, NRM)
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "ply_cloud_normals.ply"), "rb").read()
    mesh.write_mesh_ply(out, PTS, COL, FACES)
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "ply_mesh.ply"), "rb").read()
    assert fusion.write_ply is ply.write_ply and mesh.write_mesh_ply is ply.write_mesh_ply


def test_read_ply_round_trips(tmp_path):
    out = str(tmp_path / "o.ply")
    fusion.write_ply(out, PTS, COL, NRM)
    p, c = fusion.read_ply(out)                                       # used to return misaligned bytes for this file
    assert p.dtype == np.float32 and c.dtype == np.uint8 and np.array_equal(p, PTS) and np.array_equal(c, COL)
    p, c, n = fusion.read_ply_full(out)
    assert np.array_equal(p, PTS) and np.array_equal(c, COL) and np.array_equal(n, NRM)
    fusion.write_ply(out, PTS, COL)
    p, c = fusion.read_ply(out)
    assert np.array_equal(p, PTS) and np.array_equal(c, COL) and fusion.read_ply_full(out)[2] is None
    # foreign layouts raise instead of being misread: a mesh, another property order, another format, a truncated body
    mesh.write_mesh_ply(out, PTS, COL, FACES)
    with pytest.raises(ValueError, match="not a vertex layout that write_ply produces"):
        fusion.read_ply(out)
    raw = open(os.path.join(GOLDEN, "ply_cloud.ply"), "rb").read()
    open(out, "wb").write(raw.replace(b"property uchar red\nproperty uchar green\n", b"property uchar green\nproperty uchar red\n"))
    with pytest.raises(ValueError, match="not a vertex layout that write_ply produces"):
        fusion.read_ply(out)
    open(out, "wb").write(raw.replace(b"binary_little_endian", b"binary_big_endian"))
    with pytest.raises(ValueError, match="not a vertex layout that write_ply produces"):
        fusion.read_ply_full(out)
    open(out, "wb").write(raw[:-1])
    with pytest.raises(ValueError):
        fusion.read_ply(out)
    open(out, "wb").write(raw.replace(b"element vertex", b"comment a comment is accepted\nelement vertex"))
    assert np.array_equal(fusion.read_ply(out)[0], PTS)


def test_read_mesh_ply_stays_strict(tmp_path):
    out = str(tmp_path / "m.ply")
    raw = open(os.path.join(GOLDEN, "ply_mesh.ply"), "rb").read()
    open(out, "wb").write(raw)
    v, c, f = mesh.read_mesh_ply(out)
    assert np.array_equal(v, PTS) and np.array_equal(c, COL) and np.array_equal(f, FACES) and f.dtype == np.int32
    assert np.array_equal(pointcloud.read_ply_points(out), PTS)
    open(out, "wb").write(raw.replace(b"element vertex", b"comment no comments\nelement vertex"))
    with pytest.raises(ValueError, match="not the layout that write_mesh_ply produces"):
        mesh.read_mesh_ply(out)
    assert np.array_equal(pointcloud.read_ply_points(out), PTS)       # the general reader skips the comment
    head, body = raw[:raw.index(b"end_header\n") + 11], raw[raw.index(b"end_header\n") + 11:]
    quad = body[:15 * 5] + b"\x04" + body[15 * 5 + 1:]                  # the first face says it has four corners
    open(out, "wb").write(head + quad)
    with pytest.raises(ValueError, match="not triangles"):
        mesh.read_mesh_ply(out)
    open(out, "wb").write(raw[:-4])
    with pytest.raises(ValueError, match="truncated"):
        mesh.read_mesh_ply(out)
    fusion.write_ply(out, PTS, COL)                                   # a cloud is no mesh
    with pytest.raises(ValueError, match="not the layout that write_mesh_ply produces"):
        mesh.read_mesh_ply(out)


def test_uint8_colours_equal_the_float_path():
    """filter_depth keeps the image uint8 from the file to the PLY; it used to go uint8 -> float32 / 255 (host) -> * 255 ->
    uint8 (device).  The two agree for every value a pixel can have."""
    x = np.arange(256, dtype=np.uint8)
    assert np.array_equal(((x.astype(np.float32) / np.float32(255.0)) * np.float32(255.0)).astype(np.uint8), x)
    assert np.array_equal((np.asarray(x, dtype=np.float32) / 255.0 * 255).astype(np.uint8), x)
    t = torch.from_numpy(np.asarray(x, dtype=np.float32) / 255.0)     # the host division, then the device's two steps on the CPU
    assert torch.equal((t * 255).to(torch.uint8), torch.from_numpy(x))


# ------------------------------------------------------------------------------------------------------------ scan folders
SIZES = {0: (6, 8), 3: (4, 6), 7: (6, 8)}                            # view id -> (h, w): three views of two sizes


def _cam(vid):
    rng = np.random.default_rng(100 + vid)
    cam = np.zeros((2, 4, 4), np.float32)
    cam[0] = np.eye(4) + 0.1 * rng.standard_normal((4, 4))
    cam[0, 3] = (0, 0, 0, 1)
    cam[1, :3, :3] = [[361.54125, 0.0, 82.900625], [0.0, 360.3975, 66.383875], [0.0, 0.0, 1.0]]
    return cam


def _save(out, vid, h, w, scan="scan1"):
    rng = np.random.default_rng(vid)
    depth = rng.uniform(400, 900, (h, w)).astype(np.float32)
    confs = [rng.uniform(0, 1, (h, w)).astype(np.float32) for _ in range(3)]
    img = rng.uniform(0, 1, (3, h, w)).astype(np.float32)
    mvs_io.save_outputs(out, scan + "/{}/" + f"{vid:08d}" + "{}", depth, confs, _cam(vid), img)
    return depth, np.stack(confs)


def test_scan_folder_reads_what_save_outputs_wrote(tmp_path):
    from PIL import Image
    out = str(tmp_path)
    written = {vid: _save(out, vid, h, w) for vid, (h, w) in SIZES.items()}
    open(tmp_path / "scan1" / "images" / "notes.txt", "w").write("not a view")
    scan = mvs_io.ScanFolder(str(tmp_path / "scan1"))
    assert scan.view_ids() == [0, 3, 7]
    for vid, (h, w) in SIZES.items():
        d, c, img = scan.depth(vid), scan.conf(vid), scan.image(vid)
        assert d.dtype == np.float32 and d.flags["C_CONTIGUOUS"] and np.array_equal(d, written[vid][0])
        assert c.dtype == np.float32 and c.flags["C_CONTIGUOUS"] and np.array_equal(c, written[vid][1])
        assert img.dtype == np.uint8 and img.shape == (h, w, 3)
        assert np.array_equal(img, np.asarray(Image.open(scan.path("images", vid, ".jpg")).convert("RGB")))
        assert scan.map_size(vid) == (h, w) == scan.image_size(vid)
        # the camera: what the writer was given, and what render_scan / texture_scan used to assemble from read_cam_file
        cam = scan.cam(vid)
        want = _cam(vid)
        want[1, 3, 3] = 1.0
        assert cam.dtype == np.float32 and np.array_equal(cam, want)
        assert np.array_equal(cam, fusion.read_fusion_cam(scan.path("cams", vid, "_cam.txt")))
        assert fusion.read_fusion_cam is mvs_io.read_saved_cam
        intr, extr, _, _ = mvs_io.read_cam_file(scan.path("cams", vid, "_cam.txt"))
        old = np.zeros((2, 4, 4), np.float32)
        old[0], old[1, :3, :3] = extr, intr
        differ = np.argwhere(old != cam)
        assert differ.tolist() == [[1, 3, 3]] and cam[1, 3, 3] == 1     # the corner below K, which no consumer of a camera reads
    # grouping in pair order: each group in the given order, the groups by their first view
    assert scan.groups([7, 3, 0], scan.map_size) == {(6, 8): [7, 0], (4, 6): [3]}
    assert list(scan.groups([7, 3, 0], scan.map_size)) == [(6, 8), (4, 6)]
    assert list(scan.groups([3, 0, 7], scan.image_size).items()) == [((4, 6), [3]), ((6, 8), [0, 7])]
    assert scan.groups([], scan.map_size) == {}
    # a greyscale image loads as RGB
    Image.fromarray(np.full((6, 8), 77, np.uint8)).save(scan.path("images", 0, ".jpg"))
    assert scan.image(0).shape == (6, 8, 3)


def test_read_saved_cam_needs_no_depth_range_line(tmp_path):
    path = str(tmp_path / "c.txt")
    mvs_io.write_cam_file(path, _cam(1))
    lines = open(path).read().split("\n")
    open(path, "w").write("\n".join(lines[:10]) + "\n")
    want = _cam(1)
    want[1, 3, 3] = 1.0
    assert np.array_equal(mvs_io.read_saved_cam(path), want)
    with pytest.raises(IndexError):
        mvs_io.read_cam_file(path)


def test_load_views(tmp_path):
    from cds_mvsnet_amd import gipuma
    out = str(tmp_path)
    a, b = _save(out, 0, 6, 8), _save(out, 7, 6, 8)
    scan = mvs_io.ScanFolder(str(tmp_path / "scan1"))
    s = scan.load_views([7, 0])
    assert s["ids"].tolist() == [7, 0] and s["depths"].shape == (2, 6, 8) and s["confs"].shape == (2, 3, 6, 8)
    assert s["cams"].shape == (2, 2, 4, 4) and s["images"].shape == (2, 6, 8, 3) and s["images"].dtype == np.uint8
    assert np.array_equal(s["depths"], np.stack([b[0], a[0]])) and np.array_equal(s["confs"], np.stack([b[1], a[1]]))
    g = gipuma.load_scan(str(tmp_path / "scan1"))                    # every view of images/, ascending
    assert g["ids"].tolist() == [0, 7] and np.array_equal(g["depths"], s["depths"][::-1])
    _save(out, 3, 4, 6)
    with pytest.raises(ValueError, match=r"view 3 has depth \(4, 6\), confidence \(4, 6, 3\) and image \(4, 6, 3\); every view must be 6x8"):
        scan.load_views(scan.view_ids())
    os.makedirs(tmp_path / "empty" / "images")
    empty = mvs_io.ScanFolder(str(tmp_path / "empty"))
    assert empty.view_ids() == []
    with pytest.raises(ValueError, match="no views in images/"):
        empty.load_views(empty.view_ids())
    with pytest.raises(ValueError, match="no views in images/"):
        gipuma.load_scan(str(tmp_path / "empty"))


def test_read_testlist(tmp_path):
    from cds_mvsnet_amd import dtu_eval, tt_eval
    path = str(tmp_path / "list.txt")
    open(path, "w").write("\n  scan9 \n\nscan11\t\n   \nBarn")
    assert mvs_io.read_testlist(path) == ["scan9", "scan11", "Barn"]
    assert tt_eval.scene_names(path, None) == ["scan9", "scan11", "Barn"] and tt_eval.scene_names(None, " a, b,,") == ["a", "b"]
    open(path, "w").write("scan9\n\n 11\n")
    assert dtu_eval.scan_names(path, None) == ["scan9", "scan11"] == dtu_eval.scan_names(None, "9, scan11")
