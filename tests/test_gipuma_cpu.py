"""Gipuma-style fusion without a GPU: fusibile's file formats against the reference (G14), the float32 restatement of the rule
(tests/gipuma_ref.py) on hand-built scenes whose answer is known, the command lines and the device checks."""
import os

import numpy as np
import pytest
import torch

import gipuma_ref as R
from cds_mvsnet_amd import gipuma, infer, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------------------ formats
def _g14():
    return np.load(os.path.join(GOLDEN, "g14_gipuma_formats.npz"))


def _unpack(z, prefix):
    names, off, blob = z[f"{prefix}_names"], z[f"{prefix}_offsets"], z[f"{prefix}_blob"].tobytes()
    return {str(n): blob[off[i]:off[i + 1]] for i, n in enumerate(names)}


def _tree(folder):
    out = {}
    for dirpath, _, files in os.walk(folder):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


def _write_g14_scan(folder):
    z = _g14()
    for rel, data in _unpack(z, "in").items():
        os.makedirs(os.path.dirname(os.path.join(folder, rel)), exist_ok=True)
        with open(os.path.join(folder, rel), "wb") as f:
            f.write(data)
    return z


def test_export_matches_reference_bytes(tmp_path):
    """depth_est/*_prob_filtered.pfm, points_mvsnet/cams/*.P, images/, 2333__*/disp.dmb and normals.dmb byte for byte."""
    scan = str(tmp_path / "scan1")
    z = _write_g14_scan(scan)
    inputs = set(_tree(scan))
    folder = gipuma.export_fusibile_inputs(scan, tuple(z["prob_threshold"]))
    assert folder == os.path.join(scan, "points_mvsnet")
    got = {k: v for k, v in _tree(scan).items() if k not in inputs}
    want = _unpack(z, "out")
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k
    # the thresholds do something on this scan: some pixels are filtered, some are kept
    d = gipuma.read_dmb(os.path.join(folder, "2333__00000000", "disp.dmb"))
    assert 0 < int((d == 0).sum()) < d.size


def test_read_dmb_matches_reference_reader(tmp_path):
    z = _g14()
    out = _unpack(z, "out")
    for v in range(3):
        for fn in ("disp", "normals"):
            p = tmp_path / f"{fn}{v}.dmb"
            p.write_bytes(out[f"points_mvsnet/2333__{v:08d}/{fn}.dmb"])
            got, want = gipuma.read_dmb(str(p)), z[f"read_{fn}_{v}"]
            assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want), (fn, v)
            q = tmp_path / f"again{fn}{v}.dmb"
            gipuma.write_dmb(str(q), got)
            assert q.read_bytes() == p.read_bytes()


def test_read_dmb_rejects_short_payload(tmp_path):
    p = tmp_path / "bad.dmb"
    p.write_bytes(np.array([1, 4, 5, 1], "<i4").tobytes() + np.zeros(19, "<f4").tobytes())
    with pytest.raises(ValueError):
        gipuma.read_dmb(str(p))


# ------------------------------------------------------------------------------------------------ hand-built scenes
def _cam(t, f=8.0, cx=5.0, cy=3.0):
    cam = np.zeros((2, 4, 4), np.float32)
    cam[0] = np.eye(4)
    cam[0, :3, 3] = t
    cam[1, :3, :3] = [[f, 0, cx], [0, f, cy], [0, 0, 1]]
    cam[1, 3, 3] = 1.0
    return cam


def _scene(h, w, ts, pixels, cx=5.0, cy=3.0):
    """Views with E = [I | t] and K = [[8, 0, cx], [0, 8, cy], [0, 0, 1]]; every depth 0 except ``pixels``:
    (view, x, y, depth, rgb).  Confidences 1, images a fixed pattern."""
    V = len(ts)
    depths = np.zeros((V, h, w), np.float32)
    confs = np.ones((V, 3, h, w), np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    images = np.stack([np.stack([(v * 40 + xx * 3 + yy * 5) % 256, (xx * 7) % 256, (yy * 11 + v) % 256], -1)
                       for v in range(V)]).astype(np.uint8)
    for v, x, y, d, rgb in pixels:
        depths[v, y, x] = d
        if rgb is not None:
            images[v, y, x] = rgb
    return {"depths": depths, "confs": confs, "cams": np.stack([_cam(t, cx=cx, cy=cy) for t in ts]), "images": images}


def _world(cam, x, y, d):
    """float64 world point of pixel (x, y) at depth d for E = [I | t]."""
    K = cam[1, :3, :3].astype(np.float64)
    c = np.linalg.inv(K) @ np.array([x, y, 1.0]) * d
    return c - cam[0, :3, 3].astype(np.float64)


def hand_cases():
    """name -> (scene, fuse keyword arguments, check(out, scene)).  Every case is a few pixels whose answer is known."""
    cases = {}
    two = _scene(6, 10, [(0, 0, 0), (-2, 0, 0)], [(0, 6, 3, 4.0, (10, 20, 255)), (1, 2, 3, 4.01, (11, 25, 0))])

    def check_a(out, sc):       # (a) one point, the mean of both 3D points; view 1 does not emit it again
        want = (_world(sc["cams"][0], 6, 3, 4.0) + _world(sc["cams"][1], 2, 3, 4.01)) / 2
        assert out["points"].shape == (1, 3) and list(out["ref_view"]) == [0]
        np.testing.assert_allclose(out["points"][0], want, rtol=2e-6, atol=2e-6)
        used = np.zeros_like(out["used"])
        used[1, 3, 2] = True
        assert np.array_equal(out["used"], used)
    cases["a_matched_pair"] = (two, dict(num_consistent=1), check_a)

    def check_b(out, sc):       # (b) one agreeing view is not enough for num_consistent = 2
        assert out["points"].shape == (0, 3) and not out["used"].any()
    cases["b_too_few_views"] = (two, dict(num_consistent=2), check_b)

    three = _scene(6, 10, [(0, 0, 0), (-2, 0, 0), (-1, 0, 0)],
                   [(0, 6, 3, 4.0, None), (1, 2, 3, 4.0, None), (2, 4, 3, 4.0, None)])
    three["confs"][1, 1, 3, 2] = 0.4

    def check_c(out, sc):       # (c) the filtered pixel B of view 1 neither counts for A nor starts a point
        want = (_world(sc["cams"][0], 6, 3, 4.0) + _world(sc["cams"][2], 4, 3, 4.0)) / 2
        assert out["points"].shape == (1, 3) and list(out["ref_view"]) == [0]
        np.testing.assert_allclose(out["points"][0], want, rtol=2e-6, atol=2e-6)
        assert out["used"][2, 3, 4] and out["used"].sum() == 1
    cases["c_filtered_pixel"] = (three, dict(num_consistent=1, prob_threshold=(0.5, 0.5, 0.5)), check_c)

    edge = _scene(6, 10, [(0, 0, 0), (0.375, 0, 0)], [(0, 9, 3, 4.0, None), (1, 9, 3, 4.0, None)])

    def check_d_edge(out, sc):  # (d) u = 9.75 in [w - 0.5, w) samples column w - 1
        assert list(out["ref_view"]) == [0] and out["used"][1, 3, 9] and out["used"].sum() == 1
    cases["d_right_edge"] = (edge, dict(num_consistent=1), check_d_edge)

    left = _scene(6, 10, [(0, 0, 0), (-0.125, 0, 0)], [(0, 0, 3, 4.0, None), (1, 0, 3, 4.0, None)])

    def check_d_left(out, sc):  # (d) u = -0.25 does not count for view 0; view 1 sees view 0 at u = 0.25
        assert list(out["ref_view"]) == [1] and out["used"][0, 3, 0] and out["used"].sum() == 1
    cases["d_left_of_image"] = (left, dict(num_consistent=1), check_d_left)

    behind = _scene(6, 10, [(0, 0, 0), (0, 0, -5)], [(0, 5, 3, 4.0, None), (1, 5, 3, 4.0, None)])

    def check_e(out, sc):       # (e) X lies behind view 1 (z = -1, yet u, v fall inside): view 1 does not count for view 0
        assert list(out["ref_view"]) == [1]
        np.testing.assert_allclose(out["points"][0], [0.0, 0.0, 6.5], atol=2e-6)
    cases["e_behind_camera"] = (behind, dict(num_consistent=1, disp_threshold=1e6), check_e)

    chain = _scene(6, 16, [(0, 0, 0), (-0.5, 0, 0), (-4, 0, 0)],
                   [(0, 12, 3, 4.4, None), (1, 11, 3, 4.0, None), (2, 4, 3, 4.0, None)], cx=8.0)

    def check_f(out, sc):       # (f) B, used by view 0's point, still counts for view 2's pixel C (A disagrees with C)
        assert list(out["ref_view"]) == [0, 2]
        a, b, c = _world(sc["cams"][0], 12, 3, 4.4), _world(sc["cams"][1], 11, 3, 4.0), _world(sc["cams"][2], 4, 3, 4.0)
        np.testing.assert_allclose(out["points"], [(a + b) / 2, (c + b) / 2], rtol=2e-6, atol=2e-6)
        assert out["used"][1, 3, 11] and out["used"].sum() == 1
    cases["f_used_pixel_is_evidence"] = (chain, dict(num_consistent=1), check_f)

    tie = _scene(6, 10, [(0, 0, 0), (-2, 0, 0)], [(0, 6, 3, 4.0, None), (1, 2, 3, 8.0, None)])

    def check_g_equal(out, sc):  # (g) |16/4 - 16/8| = 2 exactly: not below a threshold of 2
        assert out["points"].shape == (0, 3)
    cases["g_threshold_equal"] = (tie, dict(num_consistent=1, disp_threshold=2.0), check_g_equal)

    def check_g_above(out, sc):
        assert list(out["ref_view"]) == [0]
    next_float = float(np.nextafter(np.float32(2), np.float32(3)))
    cases["g_threshold_next_float"] = (tie, dict(num_consistent=1, disp_threshold=next_float), check_g_above)

    def check_h(out, sc):       # (h) (10, 20, 255) and (11, 25, 0) -> the floor means (10, 22, 127)
        assert out["colors"].tolist() == [[10, 22, 127]]
    cases["h_colour_floor_mean"] = (two, dict(num_consistent=1), check_h)

    one = _scene(6, 10, [(0, 0, 0)], [(0, 6, 3, 4.0, None)])

    def check_i(out, sc):       # (i) a single view: nothing to agree with
        assert out["points"].shape == (0, 3) and out["colors"].shape == (0, 3) and not out["used"].any()
    cases["i_single_view"] = (one, dict(num_consistent=1), check_i)
    return cases


def run_ref(scene, **kw):
    return R.fuse(list(scene["depths"]), list(scene["confs"]), list(scene["cams"]), list(scene["images"]), **kw)


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_restatement_hand_built(name):
    scene, kw, check = hand_cases()[name]
    check(run_ref(scene, **kw), scene)


def test_restatement_rejects_mismatched_sizes():
    sc = _scene(6, 10, [(0, 0, 0), (-2, 0, 0)], [(0, 6, 3, 4.0, None)])
    depths = [sc["depths"][0], np.zeros((6, 11), np.float32)]
    with pytest.raises(ValueError):
        R.fuse(depths, list(sc["confs"]), list(sc["cams"]), list(sc["images"]))


def test_camera_constants_match_restatement():
    cams = synth.make_fusion_scene(4, 12, 16, seed=3, pixel_offset=0.0)["cams"].numpy()
    views, fb = gipuma.camera_constants(cams)
    P, M, fb_ref = R.constants(list(cams))
    for v in range(4):
        assert np.array_equal(views[v, :12].reshape(3, 4), P[v]) and np.array_equal(views[v, 12:21].reshape(3, 3), M[v])
    assert np.array_equal(fb, fb_ref) and np.all(np.diag(fb) == 0)


# ----------------------------------------------------------------------------------------------------- scene, CLIs
def test_fusion_scene_pixel_offset():
    """pixel_offset=0.5 (the default) is the existing scene; 0.0 puts the depth of pixel (x, y) at the integer coordinates."""
    a = synth.make_fusion_scene(3, 8, 12, seed=2, outlier_frac=0.0)
    b = synth.make_fusion_scene(3, 8, 12, seed=2, outlier_frac=0.0, pixel_offset=0.5)
    c = synth.make_fusion_scene(3, 8, 12, seed=2, outlier_frac=0.0, pixel_offset=0.0)
    for k in a:
        assert torch.equal(a[k], b[k])
    assert not torch.equal(a["depths"], c["depths"]) and torch.equal(a["cams"], c["cams"])
    cam = c["cams"][1].double().numpy()
    K, E = cam[1, :3, :3], cam[0]
    for x, y in ((0, 0), (11, 7), (5, 3)):
        pc = np.linalg.inv(K) @ np.array([x, y, 1.0]) * float(c["depths"][1, y, x])
        pw = np.linalg.inv(E) @ np.append(pc, 1.0)
        assert abs(pw[2] - synth.fusion_surface(pw[0], pw[1])) < 1e-3


def test_cli_parsing(tmp_path):
    a = gipuma.parse_args(["--outdir", "o", "--testlist", "l.txt"])
    assert a.prob_threshold == (0.0, 0.0, 0.0) and a.disp_threshold == 0.2 and a.num_consistent == 3 and not a.export_fusibile
    a = gipuma.parse_args(["--outdir", "o", "--testlist", "l.txt", "--prob_threshold", "0.8,0.7,0.6", "--disp_threshold", "0.1",
                           "--num_consistent", "2", "--export_fusibile"])
    assert a.prob_threshold == (0.8, 0.7, 0.6) and a.disp_threshold == 0.1 and a.num_consistent == 2 and a.export_fusibile
    with pytest.raises(ValueError):
        gipuma.parse_args(["--outdir", "o", "--testlist", "l.txt", "--prob_threshold", "0.8,0.7"])
    b = infer.parse_args(["--testpath", "t", "--testlist", "l", "--outdir", "o"])
    assert b.filter_method == "normal" and b.prob_threshold == "0.0,0.0,0.0" and b.disp_threshold == 0.2 and b.num_consistent == 3
    b = infer.parse_args(["--testpath", "t", "--testlist", "l", "--outdir", "o", "--fuse", "--filter_method", "gipuma",
                          "--disp_threshold", "0.1", "--num_consistent", "2"])
    assert b.fuse and b.filter_method == "gipuma" and b.disp_threshold == 0.1 and b.num_consistent == 2
    with pytest.raises(SystemExit):
        infer.parse_args(["--testpath", "t", "--testlist", "l", "--outdir", "o", "--filter_method", "fusibile"])


def test_fuse_views_refuses_cpu_tensors():
    sc = _scene(6, 10, [(0, 0, 0), (-2, 0, 0)], [(0, 6, 3, 4.0, None)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gipuma.fuse_views(torch.from_numpy(sc["depths"]), torch.from_numpy(sc["confs"]), sc["cams"],
                          torch.from_numpy(sc["images"]))
