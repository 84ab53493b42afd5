"""Tanks and Temples evaluation without a GPU: the readers, the declarations of the new C entry points, Umeyama from pair
sums, the reference crop on hand-worked points, the scene table and the loud refusal of host tensors."""
import json
import os
import re

import numpy as np
import pytest
import torch

import tt_eval_ref as R
from cds_mvsnet_amd import pointcloud, synth, tt_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tt_layout(root, scene, sc):
    """Write ``sc`` (synth.make_tt_scene) as <root>/<scene>/<scene>.ply, <scene>.json, <scene>_trans.txt."""
    from cds_mvsnet_amd import fusion
    d = root / scene
    os.makedirs(d, exist_ok=True)
    fusion.write_ply(str(d / f"{scene}.ply"), sc["gt"], np.zeros_like(sc["gt"], np.uint8))
    crop = sc["crop"]
    with open(d / f"{scene}.json", "w") as f:
        json.dump({"class_name": "SelectionPolygonVolume", "version_major": 1, "version_minor": 0,
                   "orthogonal_axis": crop["orthogonal_axis"], "axis_min": crop["axis_min"], "axis_max": crop["axis_max"],
                   "bounding_polygon": np.asarray(crop["bounding_polygon"]).tolist()}, f)
    with open(d / f"{scene}_trans.txt", "w") as f:
        for row in np.asarray(sc["trans"], np.float64):
            f.write(" ".join(repr(float(v)) for v in row) + "\n")


def test_readers_round_trip(tmp_path):
    sc = synth.make_tt_scene(n_gt=400, n_pred=300, seed=1)
    _tt_layout(tmp_path, "Barn", sc)
    paths = tt_eval.scene_paths(str(tmp_path), "Barn")
    assert paths["ply"] == os.path.join(str(tmp_path), "Barn", "Barn.ply")
    crop = tt_eval.read_crop(paths["crop"])
    assert crop["orthogonal_axis"] == "Z"
    assert crop["axis_min"] == sc["crop"]["axis_min"] and crop["axis_max"] == sc["crop"]["axis_max"]
    assert crop["bounding_polygon"].dtype == np.float64
    assert np.array_equal(crop["bounding_polygon"], sc["crop"]["bounding_polygon"])
    assert np.array_equal(tt_eval.read_trans(paths["trans"]), sc["trans"])           # repr round-trips float64
    assert np.array_equal(pointcloud.read_ply_points(paths["ply"]), sc["gt"])
    (tmp_path / "bad.json").write_text(json.dumps({"orthogonal_axis": "Z", "axis_min": 0, "axis_max": 1}))
    with pytest.raises(ValueError, match="bounding_polygon"):
        tt_eval.read_crop(str(tmp_path / "bad.json"))
    (tmp_path / "axis.json").write_text(json.dumps({"orthogonal_axis": "W", "axis_min": 0, "axis_max": 1,
                                                    "bounding_polygon": [[0, 0, 0], [1, 0, 0], [0, 1, 0]]}))
    with pytest.raises(ValueError, match="orthogonal_axis"):
        tt_eval.read_crop(str(tmp_path / "axis.json"))
    (tmp_path / "t.txt").write_text("1 0 0\n0 1 0\n0 0 1\n")
    with pytest.raises(ValueError, match="4x4"):
        tt_eval.read_trans(str(tmp_path / "t.txt"))


def test_new_symbols_are_declared_everywhere():
    from cds_mvsnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "cds_mvsnet_hip.h")).read()
    makefile = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "Makefile")).read()
    for name, nargs in (("cds_transform_points_f32", 5), ("cds_nn_index_f32", 15), ("cds_icp_sums_f64", 19),
                        ("cds_voxel_mean_f32", 7), ("cds_polygon_crop_f32", 9)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\);", header, re.M | re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.load(), name)
    assert re.search(r"^SRCS\s*=.*\bregistration\.hip\b", makefile, re.M)
    assert re.search(r"^%\.o:.*\bgrid_common\.hpp\b", makefile, re.M)
    csrc = os.path.join(ROOT, "cds_mvsnet_amd", "csrc")
    for src in ("registration.hip", "pointcloud.hip"):
        assert '#include "grid_common.hpp"' in open(os.path.join(csrc, src)).read(), src
    assert int(re.search(r"#define CDS_ICP_SUMS (\d+)", header).group(1)) == _lib.ICP_SUMS == R.N_SUMS
    assert int(re.search(r"#define CDS_ICP_MAX_GROUPS (\d+)", header).group(1)) == _lib.ICP_MAX_GROUPS
    assert int(re.search(r"#define CDS_CROP_MAX_VERTICES (\d+)", header).group(1)) == _lib.CROP_MAX_VERTICES


@pytest.mark.parametrize("with_scaling", [True, False])
def test_umeyama_recovers_a_known_similarity_from_exact_pairs(with_scaling):
    rs = np.random.RandomState(4)
    p = rs.uniform(-2, 3, (500, 3))
    M = synth.similarity(33.0, (0.3, -1.0, 0.5), (0.7, -1.1, 0.4), 1.37 if with_scaling else 1.0, about=(0.2, 0.1, -0.3))
    q = p @ M[:3, :3].T + M[:3, 3]
    d = p - q
    terms = np.concatenate([np.ones((500, 1)), p, q, (q[:, :, None] * p[:, None, :]).reshape(500, 9),
                            (d * d).sum(1, keepdims=True), (p * p).sum(1, keepdims=True)], 1)
    for fn in (tt_eval.umeyama, R.umeyama):
        got = fn(terms.sum(0), with_scaling)
        assert np.abs(got - M).max() < 1e-12, fn
        assert np.array_equal(got[3], [0, 0, 0, 1])
    # a reflected covariance still gives a rotation: mirror the targets
    qm = q * np.array([1.0, 1.0, -1.0])
    terms[:, 4:7] = qm
    terms[:, 7:16] = (qm[:, :, None] * p[:, None, :]).reshape(500, 9)
    for fn in (tt_eval.umeyama, R.umeyama):
        assert np.linalg.det(fn(terms.sum(0), False)[:3, :3]) > 0.999


def test_reference_pair_terms_layout():
    p = np.array([[1.0, 2.0, 3.0]], np.float32)
    q = np.array([[4.0, 6.0, 8.0]], np.float32)
    want = [1, 1, 2, 3, 4, 6, 8, 4, 8, 12, 6, 12, 18, 8, 16, 24, 9 + 16 + 25, 1 + 4 + 9]
    assert R.pair_terms(p, q)[0].tolist() == want
    t = R.pair_terms(np.repeat(p, 3, 0) * np.array([[1], [2], [3]], np.float32), np.repeat(q, 3, 0))
    assert np.array_equal(R.sum_terms(t), R.sum_terms(t, reverse=True))              # small integers: exact either way


def test_reference_crop_on_hand_worked_points_of_an_l_shape():
    # L: the square [0,2]^2 without its upper right quarter (1,2] x (1,2]
    poly = np.array([[0, 0, 0], [2, 0, 0], [2, 1, 0], [1, 1, 0], [1, 2, 0], [0, 2, 0]], np.float64)
    crop = {"orthogonal_axis": "Z", "axis_min": -1.0, "axis_max": 1.0, "bounding_polygon": poly}
    pts = np.array([[0.5, 0.5, 0.0],      # in the lower arm
                    [1.5, 0.5, 0.0],      # in the lower arm, right
                    [0.5, 1.5, 0.0],      # in the upper arm
                    [1.5, 1.5, 0.0],      # in the notch: outside
                    [2.5, 0.5, 0.0],      # right of the polygon
                    [-0.5, 0.5, 0.0],     # left of it
                    [0.5, 0.5, 1.0],      # exactly at axis_max: kept
                    [0.5, 0.5, -1.0],     # exactly at axis_min: kept
                    [0.5, 0.5, 1.0000001],   # just above axis_max (as float32: 1.00000012)
                    [0.5, 1.0, 0.0],      # v equals the vertices (2,1) and (1,1): one crossing (x = 0) is left of it
                    [1.5, 1.0, 0.0],      # on the horizontal edge y = 1: v < 1 is false at both ends, no crossing there
                    [0.5, 2.0, 0.0],      # on the top edge: not below any vertex, no edge straddles
                    [0.5, 0.0, 0.0],      # on the bottom edge: straddled by x = 0 (left) and x = 2 (right): one is left
                    ], np.float32)
    want = [True, True, True, False, False, False, True, True, False, True, False, False, True]
    assert R.crop_mask(pts, crop).tolist() == want
    # the same L seen along X and along Y
    for axis, perm in (("X", [2, 0, 1]), ("Y", [0, 2, 1])):
        c = dict(crop, orthogonal_axis=axis, bounding_polygon=poly[:, perm])
        assert R.crop_mask(pts[:, perm], c).tolist() == want, axis


def test_reference_voxel_keys_and_means():
    pts = np.array([[0.0, 0.0, 0.0], [0.1, 0.1, 0.1], [1.0, 0.0, 0.0], [0.2, 0.0, 0.4], [9.0, 0.0, 0.0]], np.float32)
    means, keys, counts = R.voxel_down_sample(pts, 0.5)            # origin -0.25: voxels (0,0,0) twice, (2,0,0), (0,0,1), (18,0,0)
    assert counts.tolist() == [2, 1, 1, 1] and (np.diff(keys) > 0).all()
    assert keys.tolist() == [0, 1, 2 << 6, (2 << 36 << 9) | (2 << 6)]
    assert np.allclose(means[0], [0.05, 0.05, 0.05]) and np.array_equal(means[1], pts[3]) and np.array_equal(means[3], pts[4])


def test_scene_table_and_tau_rule(tmp_path):
    assert tt_eval.TAU == {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003,
                           "Meetingroom": 0.01, "Truck": 0.005}
    assert tt_eval.scene_tau("Truck") == 0.005 and tt_eval.scene_tau("Truck", 0.02) == 0.02
    assert tt_eval.scene_tau("MyGarden", 0.05) == 0.05
    with pytest.raises(ValueError, match="--tau"):
        tt_eval.scene_tau("MyGarden")
    with pytest.raises(ValueError):
        tt_eval.scene_tau("Barn", 0.0)
    (tmp_path / "list.txt").write_text("Barn\n\nTruck\n")
    assert tt_eval.scene_names(str(tmp_path / "list.txt"), None) == ["Barn", "Truck"]
    assert tt_eval.scene_names(None, "Barn, Truck") == ["Barn", "Truck"]
    with pytest.raises(SystemExit):                                 # an unknown scene without --tau, before any file is read
        tt_eval.main(["--datapath", str(tmp_path), "--plydir", str(tmp_path), "--scenes", "MyGarden"])
    with pytest.raises(SystemExit):
        tt_eval.main(["--datapath", str(tmp_path), "--plydir", str(tmp_path), "--scenes", "Barn", "--device", "cpu"])


def test_host_tensors_are_refused():
    pts = torch.zeros(8, 3)
    crop = {"orthogonal_axis": "Z", "axis_min": 0.0, "axis_max": 1.0, "bounding_polygon": np.zeros((3, 3))}
    for call in (lambda: tt_eval.evaluate(pts, pts, crop, np.eye(4), 0.01),
                 lambda: tt_eval.register(pts, pts, crop, np.eye(4), 0.01),
                 lambda: tt_eval.icp(pts, pts, 0.1),
                 lambda: tt_eval.crop_points(pts, crop),
                 lambda: tt_eval.voxel_down_sample(pts, 0.1),
                 lambda: tt_eval.transform_points(pts, np.eye(4)),
                 lambda: tt_eval.pair_sums(pts, np.eye(4), pts, 0.1),
                 lambda: pointcloud.nearest_index(pts, pts, 0.1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_make_tt_scene_is_seeded_and_cut_by_its_crop():
    kw = dict(n_gt=2500, n_pred=2000, hole_radius=3.0, seed=3)         # the holes are sized in tau: small ones for a small scene
    a, b = synth.make_tt_scene(**kw), synth.make_tt_scene(**kw)
    assert np.array_equal(a["pred"], b["pred"]) and np.array_equal(a["gt"], b["gt"])
    assert a["gt"].dtype == np.float32 and a["pred"].dtype == np.float32 and a["gt"].shape == (2500, 3)
    keep = R.crop_mask(a["gt"], a["crop"])
    assert 0.3 < keep.mean() < 0.9                                  # the polygon cuts the ground truth
    aligned = R.transform(a["pred"], a["true_trans"])
    assert 0.3 < R.crop_mask(aligned, a["crop"]).mean() < 0.9       # and the prediction
    D = a["true_trans"] @ np.linalg.inv(a["trans"])
    assert 1e-4 < np.abs(D - np.eye(4)).max() < 0.05                # a small but real misalignment
    assert abs(np.cbrt(np.linalg.det(D[:3, :3])) - 1.002) < 1e-12
