"""The numpy restatement of the mesh rendering rule (render_ref.py) against things known otherwise: analytic
depths of a plane and a sphere, the watertightness of the fill rule, ties, dropped faces and hand-built integer cases."""
import os

import numpy as np
import pytest

import render_ref as R
from cds_mvsnet_amd import fit, infer, mvs_io, render

H, W = R.H, R.W
CAM = R.view_cameras(1)[0]


def _coverage(fr, h, w, sel=None):
    idx = fr["py"] * w + fr["px"]
    return np.bincount(idx if sel is None else idx[sel], minlength=h * w).reshape(h, w)


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_plane_depth_is_exact_and_covered_once():
    v, f = R.plane_mesh()
    fr = R.fragments(v, f, CAM, H, W)
    cover = _coverage(fr, H, W)
    assert cover.max() == 1 and cover.sum() > 500                          # every covered pixel by exactly one face
    out = R.render_view(v, f, CAM, H, W)
    hit = out["face"] >= 0
    assert np.array_equal(hit, cover == 1)
    assert len(np.unique(out["front"][hit])) == 1
    # the plane n_w . X = 0 in the camera frame: n_c . (Xc - t) = 0, so z = (n_c . t) / (n_c . r) along the ray r = (rx, ry, 1)
    Rm, t = R.camera_entries(CAM)[:2]
    nc = Rm @ np.array([0.3, -0.2, -1.0])
    py, px = np.nonzero(hit)
    rx, ry = R._rays(CAM, px, py)
    za = (nc @ t) / (nc[0] * rx + nc[1] * ry + nc[2])
    err = np.abs(out["depth"][hit].astype(np.float64) - za) / _ulp32(za)
    print(f"plane: {hit.sum()} pixels, largest depth error {err.max():.3f} fp32 ulp")
    assert err.max() <= 1.0


def test_closed_sphere_is_watertight_and_between_its_spheres():
    v, f = R.uv_sphere()
    fr = R.fragments(v, f, CAM, H, W)
    nf, nb = _coverage(fr, H, W, fr["front"]), _coverage(fr, H, W, ~fr["front"])
    covered = (nf + nb) > 0
    assert covered.sum() > 500
    assert np.array_equal(nf[covered], np.ones(covered.sum(), int)) and np.array_equal(nb[covered], np.ones(covered.sum(), int))
    out = R.render_view(v, f, CAM, H, W)
    hit = out["face"] >= 0
    assert np.array_equal(hit, covered) and (out["front"][hit] == 1).all() and np.array_equal(out["valid"], out["front"])
    Rm, t = R.camera_entries(CAM)[:2]
    za, sil = R.ray_sphere_depth(CAM, t, float(np.float32(R.SPHERE_R)), H, W)
    assert not (hit & ~sil).any()                                           # a subset of the analytic silhouette
    # the inscribed sphere: the smallest distance from the centre to a face plane
    _, _, _, Xc = R.project(v, CAM)
    n, d = R._planes(Xc, f.astype(np.int64))
    r_in = (np.abs(d - n @ t) / np.linalg.norm(n, axis=1)).min()
    assert 0.9 * R.SPHERE_R < r_in < R.SPHERE_R
    z_in, hit_in = R.ray_sphere_depth(CAM, t, r_in, H, W)
    py, px = np.nonzero(hit)
    rx, ry = R._rays(CAM, px, py)
    ray = np.stack([rx, ry, np.ones_like(rx)], 1)
    nw = n[out["face"][hit]]
    cosi = np.abs((nw * ray).sum(1)) / (np.linalg.norm(nw, axis=1) * np.linalg.norm(ray, axis=1))
    sel = cosi >= 0.2
    depth = out["depth"][hit].astype(np.float64)
    slack = 4.0 * _ulp32(depth)
    assert sel.sum() > 400
    assert (za[hit][sel] <= depth[sel] + slack[sel]).all()
    inner = sel & hit_in[hit]
    assert inner.sum() > 400 and (depth[inner] <= z_in[hit][inner] + slack[inner]).all()


def test_coincident_faces_give_the_lower_index():
    v, f = R.plane_mesh()
    one = R.render_view(v, f, CAM, H, W)
    two = R.render_view(v, np.concatenate([f, f]), CAM, H, W)
    rev = R.render_view(v, np.concatenate([f[::-1], f]), CAM, H, W)
    assert np.array_equal(two["face"], one["face"]) and np.array_equal(two["depth"].view(np.uint32), one["depth"].view(np.uint32))
    hit = one["face"] >= 0
    assert np.array_equal(rev["face"][hit], len(f) - 1 - one["face"][hit])


def test_a_vertex_behind_the_camera_drops_the_face():
    cam = R.pixel_camera()
    v = np.array([[1.0, 1.0, 1.0], [9.0, 1.0, 1.0], [1.0, 9.0, 1.0], [1.0, 9.0, 0.0], [1.0, 9.0, -1.0]], np.float32)
    assert (R.render_view(v, [(0, 1, 2)], cam, 12, 12)["face"] >= 0).sum() > 20
    for last in (3, 4):
        out = R.render_view(v, [(0, 1, last)], cam, 12, 12)
        assert (out["face"] == -1).all() and (out["depth"] == 0).all() and (out["valid"] == 0).all()


def test_the_wild_mesh_has_every_kind_of_unusable_vertex():
    """What test_render_gpu relies on: in view 0 the extra vertices of wild_mesh() fail rule 1 each in its own way, one is usable
    far outside the map, and the large face is drawn behind the plane."""
    v, f = R.wild_mesh()
    n = len(R.plane_mesh()[0])
    X, Y, usable, Xc = R.project(v, CAM)
    assert usable[:n].all() and Xc[n, 2] <= 0 and not usable[n]                              # behind the camera
    assert not usable[[n + 2, n + 4, n + 5]].any() and not np.isfinite(Xc[n + 4:n + 6]).any(1).all()   # 1e30 behind, inf, NaN
    assert usable[n + 3] and Xc[n + 3, 2] > 1e29 and Y[n + 3] > 256 * H                     # 1e30 away, in front, off the map
    assert usable[n + 9] and X[n + 9] < -256 * 2 * W                                         # usable, far outside the map
    assert Xc[n + 10, 2] > 0 and not usable[n + 10]                                          # finite, in front, beyond 2^28
    out = R.render_view(v, f, CAM, H, W)
    large = len(R.plane_mesh()[1]) + 7
    assert (out["face"] == large).sum() > 300 and (out["face"] >= 0).sum() > (out["face"] == large).sum() + 2000


def test_reversing_a_face_flips_front_only():
    v, f = R.uv_sphere()
    a = R.render_view(v, f, CAM, H, W)
    b = R.render_view(v, f[:, [0, 2, 1]], CAM, H, W)
    hit = a["face"] >= 0
    assert np.array_equal(a["face"], b["face"]) and np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))
    assert (a["front"][hit] == 1).all() and (b["front"][hit] == 0).all() and (b["front"][~hit] == 0).all()
    assert (b["valid"] == 0).all()


def test_top_left_rule_on_pixel_centres():
    """Vertices on pixel centres, edges through pixel centres (K = 1, z = 1: u = x exactly).  The triangle (0.5, 0.5), (4.5, 0.5),
    (0.5, 4.5) owns its top and left edges and not its hypotenuse; its neighbour across the hypotenuse owns that edge (a left edge
    for it) and not its right and bottom edges: the 4 x 4 square is covered exactly once."""
    cam = R.pixel_camera()
    v = np.array([[0.5, 0.5, 1.0], [4.5, 0.5, 1.0], [0.5, 4.5, 1.0], [4.5, 4.5, 1.0]], np.float32)
    X, Y, usable, _ = R.project(v, cam)
    assert usable.all() and X.tolist() == [128, 1152, 128, 1152] and Y.tolist() == [128, 128, 1152, 1152]
    py, px = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    for tri in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        got = R.render_view(v, [tri], cam, 8, 8)["face"] == 0
        assert np.array_equal(got, px + py <= 3), tri
    for tri in ((1, 3, 2), (2, 3, 1)):
        got = R.render_view(v, [tri], cam, 8, 8)["face"] == 0
        assert np.array_equal(got, (px + py >= 4) & (px <= 3) & (py <= 3)), tri
    fr = R.fragments(v, [(0, 1, 2), (1, 3, 2)], cam, 8, 8)
    assert np.array_equal(_coverage(fr, 8, 8), ((px <= 3) & (py <= 3)).astype(int))
    # a horizontal bottom edge and a vertical right edge through pixel centres are not owned
    got = R.render_view(v, [(0, 1, 3)], cam, 8, 8)["face"] == 0                  # top edge y = 0.5, right edge x = 4.5
    assert np.array_equal(got, (py <= px) & (px <= 3))                            # the diagonal is its left edge: owned
    # a triangle that contains no pixel centre draws nothing
    tiny = np.array([[1.1, 1.1, 1.0], [1.4, 1.1, 1.0], [1.1, 1.4, 1.0]], np.float32)
    assert (R.render_view(tiny, [(0, 1, 2)], cam, 8, 8)["face"] == -1).all()


def test_colours_interpolate_and_miss_is_black():
    v, f = R.plane_mesh()
    c = np.full((len(v), 3), 77, np.uint8)
    out = R.render_view(v, f, CAM, H, W, c)
    hit = out["face"] >= 0
    assert (out["image"][hit] == 77).all() and (out["image"][~hit] == 0).all()   # the weights sum to one
    out = R.render(v, f, R.view_cameras(2), H, W, R.vertex_colors(len(v)))
    assert out["image"].shape == (2, H, W, 3) and out["image"][out["face"] >= 0].std() > 10


# ---------------------------------------------------------------------------------------------------------- command lines
def test_render_mesh_needs_mesh_voxel(capsys):
    args = ["--testpath", "x", "--testlist", "y", "--outdir", "z", "--fuse"]
    for extra in (["--render_mesh"], ["--mesh_voxel", "10", "--export_blended", "d"], ["--mesh_voxel", "10", "--render_mesh",
                                                                                         "--max_rel_diff", "-1"]):
        with pytest.raises(SystemExit):
            infer.parse_args(args + extra)
    capsys.readouterr()
    a = infer.parse_args(args + ["--mesh_voxel", "10", "--render_mesh", "--back", "keep", "--max_rel_diff", "0.01"])
    assert a.render_mesh and a.back == "keep" and a.max_rel_diff == 0.01 and a.export_blended is None and not a.save_image
    assert not infer.parse_args(args).render_mesh


def test_fit_takes_a_crop(capsys):
    base = ["--dataset", "blended", "--datapath", "d", "--trainlist", "l"]
    assert fit.parse_args(base).crop is None and fit.parse_args(base + ["--crop", "128,160"]).crop == [128, 160]
    for bad in ("128", "0,160", "a,b"):
        with pytest.raises(SystemExit):
            fit.parse_args(base + ["--crop", bad])
    capsys.readouterr()


def test_export_blended_writes_the_training_tree(tmp_path):
    """Matrices from the output folder's camera file, the depth-range line from the scene's; images and maps as bytes."""
    scene, out, dst = tmp_path / "scenes" / "s", tmp_path / "out" / "s", tmp_path / "dst"
    for d in (scene / "cams", out / "cams", out / "images", out / "depth_mesh"):
        os.makedirs(d)
    cam = R.view_cameras(2)
    for i in range(2):
        mvs_io.write_cam_file(str(out / "cams" / f"{i:08d}_cam.txt"), cam[i])
        with open(scene / "cams" / f"{i:08d}_cam.txt", "w") as f:
            f.write("extrinsic\n1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n\nintrinsic\n9 0 9\n0 9 9\n0 0 1\n" +
                    f"\n{400 + i}.5 1.25 96 {520 + i}.5\n")
        (out / "images" / f"{i:08d}.jpg").write_bytes(b"jpeg %d" % i)
        mvs_io.write_pfm(str(out / "depth_mesh" / f"{i:08d}.pfm"), np.full((3, 4), 7.0 + i, np.float32))
    (scene / "pair.txt").write_text("2\n0\n1 1 1.0\n1\n1 0 1.0\n")
    assert render.export_blended("s", str(tmp_path / "scenes"), str(tmp_path / "out"), str(dst)) == 2
    for i in range(2):
        intr, extr, dmin, dint = mvs_io.read_cam_file(str(dst / "s" / "cams" / f"{i:08d}_cam.txt"), ndepths=96)
        assert np.array_equal(intr, cam[i][1, :3, :3]) and np.array_equal(extr, cam[i][0]) and (dmin, dint) == (400.5 + i, 1.25)
        lines = (dst / "s" / "cams" / f"{i:08d}_cam.txt").read_text().splitlines()
        assert lines[11] == f"{400 + i}.5 1.25 96 {520 + i}.5" and len(lines) == 12
        assert (dst / "s" / "blended_images" / f"{i:08d}.jpg").read_bytes() == b"jpeg %d" % i
        assert mvs_io.read_pfm(str(dst / "s" / "rendered_depth_maps" / f"{i:08d}.pfm"))[0][0, 0] == 7.0 + i
    assert (dst / "s" / "cams" / "pair.txt").read_text() == (scene / "pair.txt").read_text()
    os.remove(scene / "cams" / "00000001_cam.txt")
    with pytest.raises(FileNotFoundError):
        render.export_blended("s", str(tmp_path / "scenes"), str(tmp_path / "out"), str(dst))
