"""COLMAP -> MVSNet conversion, host side: the model readers and writers, the float64 restatement (tests/colmap_ref.py)
and the package's file writers against the files the REFERENCE's colmap2mvsnet.py wrote for the G15 model
(tests/golden/make_golden_colmap.py), and the errors and CLI defaults.  The kernels are tested in test_colmap_gpu.py."""
import os

import numpy as np
import pytest

import colmap_ref as R
from cds_mvsnet_amd import colmap, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_colmap.npz")
RUNS = [(".txt", 192), (".txt", 0), (".bin", 192), (".bin", 0)]


def unpack(z, prefix):
    names, off, blob = z[prefix + "_names"], z[prefix + "_offsets"], z[prefix + "_blob"].tobytes()
    return {str(n): blob[off[i]:off[i + 1]] for i, n in enumerate(names)}


def fixture():
    z = np.load(GOLDEN)
    out = {"model": unpack(z, "model"), "images": unpack(z, "images")}
    for ext, max_d in RUNS:
        out[(ext, max_d)] = unpack(z, f"out_{ext[1:]}_{max_d}")
        out[("ties", ext, max_d)] = z[f"out_{ext[1:]}_{max_d}_tied_ids"]
    return out


def write_dense(folder, fx):
    """The fixture's COLMAP dense folder (images/ and sparse/ in both formats) under ``folder``."""
    for group in ("model", "images"):
        for name, data in fx[group].items():
            p = os.path.join(folder, name)
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as f:
                f.write(data)
    return folder


def fixture_model(tmp_path, ext=".bin"):
    fx = fixture()
    return colmap.read_model(os.path.join(write_dense(str(tmp_path / "dense"), fx), "sparse"), ext), fx


def assert_models_equal(a, b):
    (ca, ia, pa), (cb, ib, pb) = a, b
    assert list(ca) == list(cb) and list(ia) == list(ib)
    for k in ca:
        assert ca[k][:4] == cb[k][:4] and np.array_equal(ca[k].params, cb[k].params)
    for k in ia:
        assert (ia[k].id, ia[k].camera_id, ia[k].name) == (ib[k].id, ib[k].camera_id, ib[k].name)
        for f in ("qvec", "tvec", "xys", "point3D_ids"):
            x, y = getattr(ia[k], f), getattr(ib[k], f)
            assert x.dtype == y.dtype and np.array_equal(x, y), (k, f)
    assert pa == pb


def scene_files(folder):
    out = {}
    for dirpath, _, files in os.walk(folder):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, folder).replace(os.sep, "/")] = open(p, "rb").read()
    return out


# ------------------------------------------------------------------------------------------------------- 1. model IO
def test_text_and_binary_models_are_equal(tmp_path):
    (txt, fx) = fixture_model(tmp_path, ".txt")
    binm = colmap.read_model(str(tmp_path / "dense" / "sparse"), ".bin")
    assert_models_equal(txt, binm)
    cameras, images, points = binm
    assert len(images) == 12 and len(points) == 400 and {c.model for c in cameras.values()} == {"PINHOLE", "SIMPLE_RADIAL"}
    ids = sorted(images)
    assert ids != list(range(ids[0], ids[0] + 12)) and list(images) != ids          # gaps, and not stored in id order
    assert any((im.point3D_ids == -1).any() for im in images.values())
    valid = [im.point3D_ids[im.point3D_ids != -1] for im in images.values()]
    assert any(np.unique(v).size < v.size for v in valid) and min(v.size for v in valid) <= 3   # duplicates; isolated image


@pytest.mark.parametrize("ext", [".txt", ".bin"])
def test_write_model_round_trips(tmp_path, ext):
    model, fx = fixture_model(tmp_path, ext)
    out = str(tmp_path / "again")
    colmap.write_model(out, ext, *model)
    assert_models_equal(colmap.read_model(out, ext), model)
    for name in ("cameras", "images", "points3D"):                 # the fixture's files came from the same writer
        assert open(os.path.join(out, name + ext), "rb").read() == fx["model"][f"sparse/{name}{ext}"]
    other = ".bin" if ext == ".txt" else ".txt"
    colmap.write_model(out, other, *model)
    assert_models_equal(colmap.read_model(out, other), model)


def test_camera_model_table():
    want = {"SIMPLE_PINHOLE": 3, "PINHOLE": 4, "SIMPLE_RADIAL": 4, "RADIAL": 5, "OPENCV": 8, "OPENCV_FISHEYE": 8,
            "FULL_OPENCV": 12, "FOV": 5, "SIMPLE_RADIAL_FISHEYE": 4, "RADIAL_FISHEYE": 5, "THIN_PRISM_FISHEYE": 12}
    assert {name: n for name, n in colmap.CAMERA_MODELS.values()} == want and sorted(colmap.CAMERA_MODELS) == list(range(11))
    for name, n in want.items():
        p = np.arange(1.0, n + 1)
        K = colmap.intrinsic_matrix(colmap.Camera(1, name, 10, 10, p))
        one_f = name in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL", "RADIAL_FISHEYE")
        assert np.array_equal(K, [[1, 0, 2], [0, 1, 3], [0, 0, 1]] if one_f else [[1, 0, 3], [0, 2, 4], [0, 0, 1]]), name


def test_bulk_reader_reads_a_large_binary_model(tmp_path):
    """3 * 10^5 points / 1.8 * 10^6 observations in binary, read back equal.  The readers work in bulk (frombuffer per image,
    gathers per block of points): this takes about a second; the bound of a minute only catches a per-observation Python loop
    (the reference's reader needs minutes here) and leaves a loaded machine a factor of ~50."""
    import time
    model = synth.make_colmap_model(100, 300_000, seed=3, min_angle_deg=None)
    colmap.write_model(str(tmp_path), ".bin", *model)
    t0 = time.time()
    back = colmap.read_model(str(tmp_path), ".bin")
    took = time.time() - t0
    assert_models_equal(back, model)
    assert sum(len(im.point3D_ids) for im in back[1].values()) > 1_500_000
    assert took < 60.0, took


# ---------------------------------------------------------------------------- 1./2. the rule against the reference
@pytest.mark.parametrize("ext,max_d", RUNS)
def test_restatement_reproduces_reference_files(tmp_path, ext, max_d):
    model, fx = fixture_model(tmp_path, ext)
    s = R.scene(*model, max_d=max_d)
    got = {"cams/%08d_cam.txt" % i: R.cam_text(s["ext"][i], s["intr"][i], s["ranges"][i]).encode() for i in range(len(s["ext"]))}
    got["pair.txt"] = R.pair_text(s["view_sel"]).encode()
    want = fx[(ext, max_d)]
    R.assert_same_scene_files(got, want)
    assert len(fx[("ties", ext, max_d)]) > 0                        # the tie rule is exercised
    assert sorted(k for k in want if k.startswith("images_post/")) == ["images_post/%08d.jpg" % i for i in range(12)]


@pytest.mark.parametrize("ext,max_d", RUNS)
def test_package_writers_reproduce_reference_files(tmp_path, ext, max_d):
    """Host functions only: cameras, the depth-range line (both max_d branches), the selection and the two writers, fed with
    the restatement's score matrix and (depth_min, depth_max)."""
    model, fx = fixture_model(tmp_path, ext)
    s = R.scene(*model, max_d=max_d)
    e, k, c = colmap.scene_cameras(model[0], model[1])
    assert np.array_equal(e, s["ext"]) and np.array_equal(k, s["intr"]) and np.abs(c - s["centres"]).max() < 1e-13
    ranges = colmap.finish_depth_ranges(s["min_max"], e, k, max_d, 1.0)
    save = str(tmp_path / "scene")
    os.makedirs(os.path.join(save, "cams"))
    open(os.path.join(save, "cams", "stale.txt"), "w").write("x")
    colmap.write_scene(save, e, k, ranges, s["score"])
    colmap.convert_images(str(tmp_path / "dense" / "images"), save, model[1])
    got = scene_files(save)
    assert "cams/stale.txt" not in got                              # cams/ is replaced
    R.assert_same_scene_files(got, fx[(ext, max_d)])
    for name, data in fx[(ext, max_d)].items():
        if name.startswith("images_post/"):
            assert got[name] == data                                # .jpg images are copied byte for byte


def test_select_views_order():
    score = np.array([[0, 3, 3, 1, 0], [3, 0, 2, 2, 2], [3, 2, 0, 0, 0], [1, 2, 0, 0, 5], [0, 2, 0, 5, 0]], np.float64)
    sel = colmap.select_views(score)
    assert [k for k, _ in sel[0]] == [2, 1, 3, 4, 0]                # ties: higher index first; k = i (score 0) is kept
    assert [k for k, _ in sel[1]] == [0, 4, 3, 2, 1]
    big = np.arange(144, dtype=np.float64).reshape(12, 12)
    assert [len(r) for r in colmap.select_views(big)] == [10] * 12 and colmap.select_views(big)[0][0] == (11, 11.0)


def test_non_jpg_images_are_reencoded(tmp_path):
    from PIL import Image
    model, _ = fixture_model(tmp_path)
    images = {k: im._replace(name=im.name.replace(".jpg", ".png")) for k, im in model[1].items()}
    src = tmp_path / "png"
    os.makedirs(src)
    for im in images.values():
        Image.fromarray(np.full((8, 12, 3), im.id % 256, np.uint8)).save(str(src / im.name))
    colmap.convert_images(str(src), str(tmp_path / "scene"), images)
    for i, iid in enumerate(sorted(images)):
        with Image.open(str(tmp_path / "scene" / "images_post" / ("%08d.jpg" % i))) as im:
            assert im.format == "JPEG" and im.size == (12, 8) and abs(int(np.asarray(im)[0, 0, 0]) - iid % 256) <= 2


# ------------------------------------------------------------------------------------------ 3. errors and arguments
def test_empty_image_raises(tmp_path):
    (cameras, images, points), _ = fixture_model(tmp_path)
    k = sorted(images)[4]
    images[k] = images[k]._replace(point3D_ids=np.full_like(images[k].point3D_ids, -1))
    with pytest.raises(ValueError, match=images[k].name):
        colmap.flatten_observations(images, points)


def test_dangling_point_id_raises(tmp_path):
    (cameras, images, points), _ = fixture_model(tmp_path)
    k = sorted(images)[2]
    ids = images[k].point3D_ids.copy()
    ids[np.nonzero(ids != -1)[0][0]] = int(points.ids.max()) + 7
    images[k] = images[k]._replace(point3D_ids=ids)
    with pytest.raises(ValueError, match=str(int(points.ids.max()) + 7)):
        colmap.flatten_observations(images, points)


def test_save_folder_equal_to_dense_folder_raises(tmp_path):
    dense = write_dense(str(tmp_path / "dense"), fixture())
    with pytest.raises(ValueError, match="dense folder"):
        colmap.main(["--dense_folder", dense, "--save_folder", os.path.join(dense, "..", "dense")])
    assert sorted(os.listdir(dense)) == ["images", "sparse"]         # nothing was touched


def test_cli_defaults_are_the_references():
    a = colmap.parse_args(["--dense_folder", "d", "--save_folder", "s"])
    assert (a.max_d, a.interval_scale, a.theta0, a.sigma1, a.sigma2, a.model_ext) == (192, 1, 5, 1, 10, ".bin")
    b = colmap.parse_args(["--dense_folder", "d", "--save_folder", "s", "--max_d", "0", "--interval_scale", "1.06", "--theta0", "4"])
    assert (b.max_d, b.interval_scale, b.theta0) == (0, 1.06, 4.0) and isinstance(b.max_d, int)
    with pytest.raises(SystemExit):
        colmap.parse_args(["--dense_folder", "d", "--save_folder", "s", "--model_ext", ".ply"])
    with pytest.raises(SystemExit):
        colmap.parse_args(["--save_folder", "s"])


def test_cpu_tensors_raise():
    """No CPU fallback: the kernels' wrappers refuse host tensors (before the library is even loaded)."""
    import torch
    from cds_mvsnet_amd import ops
    z = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="device tensor"):
        ops.colmap_pair_scores(z, z.long(), torch.zeros(2, 3, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64), 5, 1, 10)
    with pytest.raises(ValueError, match="device tensor"):
        ops.colmap_depth_ranges(z, z.long(), torch.zeros(2, 3, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.float64),
                                torch.ones(3, dtype=torch.int32), torch.ones(3, dtype=torch.int32))


def test_generator_options():
    cameras, images, points = synth.make_colmap_model(64, 20_000, seed=1, dup_frac=0.01)       # asserts theta >= 0.1
    L = np.diff(points.track_ptr)
    assert 5.0 < L.mean() < 7.0 and L.max() == 62 and (L == 2).any() and (L[L > 0] >= 1).all()
    assert (L > 31).sum() > 50                                             # the long tail: ~1 % of the tracks, uniform in [2, 62]
    ids = sorted(images)
    assert (np.diff(ids) > 1).any() and (np.diff(points.ids) > 1).any() and list(images) != ids      # gaps; shuffled dict
    valid = [images[k].point3D_ids[images[k].point3D_ids != -1] for k in ids]
    assert [v.size for v in valid[-2:]] == [3, 3] and min(v.size for v in valid[:-2]) > 100   # the two almost-isolated images
    assert all((images[k].point3D_ids == -1).sum() >= 2 for k in ids)                         # -1 observations everywhere
    dups = sum(v.size - np.unique(v).size for v in valid)
    assert 0.005 * L.sum() < dups < 0.015 * L.sum()                                          # dup_frac = 0.01
    tracked = sum(v.size for v in valid) - dups
    assert tracked == L.sum()                                                                  # duplicates are not in a track
    assert {images[k].camera_id for k in ids} == {1, 3}
    assert not any(np.unique(v).size < v.size for v in
                   (im.point3D_ids[im.point3D_ids != -1] for im in synth.make_colmap_model(8, 200, seed=1)[1].values()))
    with pytest.raises(AssertionError, match="triangulation angle"):
        synth.make_colmap_model(64, 2000, seed=1, min_angle_deg=5.0)
