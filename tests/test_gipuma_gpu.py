"""Gipuma-style fusion on the MI355X: the kernels against the float32 restatement (tests/gipuma_ref.py) bit for bit, the
hand-built cases, determinism and streams, no host synchronisation per view, the geometry of the fused points, infer and
the CLI end to end, and DTU accuracy / completeness of a fused scan."""
import os
import warnings

import numpy as np
import pytest
import torch

import dtu_eval_ref as DR
import gipuma_ref as R
from cds_mvsnet_amd import dtu_eval, fusion, gipuma, infer, mvs_io, pointcloud, synth
from test_gipuma_cpu import hand_cases, run_ref
from test_mvs_io import _write_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROB = (0.1, 0.05, 0.1)


def _run(scene, **kw):
    out = gipuma.fuse_views(torch.from_numpy(np.ascontiguousarray(scene["depths"])).to(DEV),
                            torch.from_numpy(np.ascontiguousarray(scene["confs"])).to(DEV), scene["cams"],
                            torch.from_numpy(np.ascontiguousarray(scene["images"])).to(DEV), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_bitwise(got, want):
    assert got["points"].shape == want["points"].shape, (got["points"].shape, want["points"].shape)
    assert np.array_equal(got["points"].view(np.uint32), want["points"].view(np.uint32))
    assert np.array_equal(got["colors"], want["colors"])
    assert np.array_equal(got["ref_view"], want["ref_view"])
    assert np.array_equal(got["used"], want["used"])


def _synthetic(V, h, w, seed=0):
    sc = synth.make_fusion_scene(V, h, w, seed=seed, pixel_offset=0.0)
    return {"depths": sc["depths"].numpy(), "confs": sc["confs"].numpy(), "cams": sc["cams"].numpy(),
            "images": (sc["imgs"].numpy() * 255).astype(np.uint8)}


@pytest.mark.parametrize("disp,ncons", [(0.1, 2), (0.4, 3), (1.0, 1)])
@pytest.mark.parametrize("V,h,w", [(3, 37, 53), (7, 64, 80), (12, 120, 160), (49, 96, 128)])
def test_kernel_matches_restatement_bitwise(V, h, w, disp, ncons):
    sc = _synthetic(V, h, w, seed=V)
    kw = dict(prob_threshold=PROB, disp_threshold=disp, num_consistent=ncons)
    got, want = _run(sc, **kw), run_ref(sc, **kw)
    if ncons < V:
        assert want["points"].shape[0] > 0.05 * h * w and want["used"].any()
    else:                                                 # fewer other views than num_consistent: nothing can be emitted
        assert want["points"].shape[0] == 0
    _assert_bitwise(got, want)


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_built_cases(name):
    scene, kw, check = hand_cases()[name]
    got = _run(scene, **kw)
    check(got, scene)
    _assert_bitwise(got, run_ref(scene, **kw))


def test_mismatched_sizes_raise(tmp_path):
    sc = _synthetic(3, 16, 20)
    with pytest.raises(ValueError):
        gipuma.fuse_views(torch.from_numpy(sc["depths"]).to(DEV), torch.from_numpy(sc["confs"][:, :, :15]).contiguous().to(DEV),
                          sc["cams"], torch.from_numpy(sc["images"]).to(DEV))
    scan = tmp_path / "scan1"
    _write_infer_folder(scan, sc)
    mvs_io.write_pfm(str(scan / "depth_est" / "00000001.pfm"), np.zeros((16, 21), np.float32))
    with pytest.raises(ValueError):
        gipuma.filter_scan(str(scan), str(tmp_path / "scan1.ply"))


def test_repeatable_and_side_stream():
    sc = _synthetic(7, 64, 80, seed=2)
    kw = dict(prob_threshold=PROB, disp_threshold=0.4, num_consistent=2)
    a, b = _run(sc, **kw), _run(sc, **kw)
    _assert_bitwise(a, b)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = _run(sc, **kw)
    s.synchronize()
    _assert_bitwise(a, c)
    assert a["points"].shape[0] > 0


def _sync_warnings(V):
    sc = _synthetic(V, 48, 64, seed=V)
    args = (torch.from_numpy(sc["depths"]).to(DEV), torch.from_numpy(sc["confs"]).to(DEV), sc["cams"],
            torch.from_numpy(sc["images"]).to(DEV))
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = gipuma.fuse_views(*args, num_consistent=2)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert out["points"].shape[0] > 0
    return [str(w.message).splitlines()[0] for w in rec if "synchroniz" in str(w.message)]


def test_no_host_sync_per_view():
    """The host waits a fixed number of times per scan (constant uploads and the point count), not once per view.  The
    first call is a warm-up: it may add waits of its own (first use of the allocator's block sizes)."""
    _sync_warnings(3)
    w3, w12 = _sync_warnings(3), _sync_warnings(12)
    assert len(w3) == len(w12) and 1 <= len(w12) <= 3, (w3, w12)


def _outlier_scene():
    """The fusion scene of 5 views at 240x320 (seed 4) with pixel_offset 0 and its 15 % outlier pixels, whose depth error
    is set per view to +2, -3, +4, -5, +6 %: every outlier lies in synth's +-2..6 % range, and two outliers of different
    views never agree (they differ by at least 2 % in depth)."""
    sc = synth.make_fusion_scene(5, 240, 320, seed=4, pixel_offset=0.0)
    clean = synth.make_fusion_scene(5, 240, 320, seed=4, pixel_offset=0.0, outlier_frac=0.0)["depths"]
    bad = sc["depths"] != clean
    for v in range(5):
        sc["depths"][v] = torch.where(bad[v], clean[v] * (1.0 + (-1) ** v * (0.02 + 0.01 * v)), clean[v])
    return {"depths": sc["depths"].numpy(), "confs": sc["confs"].numpy(), "cams": sc["cams"].numpy(),
            "images": (sc["imgs"].numpy() * 255).astype(np.uint8)}, bad


def test_points_lie_on_the_surface():
    """At (disp 0.1, 2 views) every emitted point is the mean of inlier samples, so it lies on Z = fusion_surface(X, Y).

    Bound.  A sample is the exact surface point of its pixel (depth rendered in float64), up to fp32 rounding (< 1e-3 here).
    All samples of a point fall within sqrt(2)/2 pixel of X's projection: at z <= 700 and f = 288 that is 1.72 units, so two
    samples lie at most 2 x 1.72 x 1.1 = 3.8 units apart in (X, Y) (the 1.1 covers the tilt of the views).  The mean of
    points on a surface with Hessian norm <= 40 sqrt(1/60^4 + 1/50^4 + 2/3000^2) = 0.0271 departs from it by at most
    0.5 x 0.0271 x 3.8^2 = 0.20, so the bound is 0.25.  One outlier sample (2-6 % of 610-690) moves the mean of at most 5
    samples by >= 0.02 x 610 / 5 = 2.4 units: ten times the bound.  The scene makes every outlier fail the disparity test
    (min over pairs of fb / z x 0.0196 = 0.137 > 0.1, checked below), so none may enter."""
    sc, bad = _outlier_scene()
    views, fb = gipuma.camera_constants(sc["cams"])
    assert (fb + np.eye(5, dtype=np.float32) * 1e9).min() / 690.0 * 0.0196 > 0.13
    out = _run(sc, disp_threshold=0.1, num_consistent=2)
    p = out["points"].astype(np.float64)
    assert p.shape[0] > 0.8 * 240 * 320 and bad.float().mean() > 0.1
    dev = np.abs(p[:, 2] - synth.fusion_surface(p[:, 0], p[:, 1]))
    assert dev.max() < 0.25, dev.max()
    assert set(np.unique(out["ref_view"])) == set(range(5))


def test_dtu_accuracy_completeness():
    """evaluate() on the fused scan of test_points_lie_on_the_surface against make_dtu_scene ground truth (STL on a
    jittered 3-unit grid over |X| <= 300, |Y| <= 220; mask voxels of 8; thinning at 2).  A point on the surface is on
    average ~0.38 pitch from the nearest jittered grid sample (1.1 units; the slope adds a little), so the medians sit near
    1.1-1.4: bounds 1.6.  The mask reaches 36 units beyond the STL in Y, where the distances grow up to the 20 cap, so the
    accuracy mean may reach 2.5; completeness sees no such band (every STL point is inside view 0): mean < 1.6."""
    sc, _ = _outlier_scene()
    out = gipuma.fuse_views(*(torch.from_numpy(np.ascontiguousarray(sc[k])).to(DEV) for k in ("depths", "confs")), sc["cams"],
                            torch.from_numpy(sc["images"]).to(DEV), disp_threshold=0.1, num_consistent=2)
    gt = synth.make_dtu_scene(300, 220, 3.0, 8.0, 20.0, plane_z=640.0)
    r = dtu_eval.evaluate(out["points"], gt, dst=2.0, max_dist=20.0, seed=0)
    assert 0.5 < r["acc_median"] < 1.6 and 0.5 < r["acc"] < 2.5, r
    assert 0.5 < r["comp_median"] < 1.6 and 0.5 < r["comp"] < 1.6, r
    want = DR.point_compare(out["points"].cpu().numpy(), gt, 2.0, pointcloud.thinning_order(out["points"].shape[0], 0).numpy(),
                            max_dist=20.0, block=60.0)
    assert abs(r["acc"] - want["acc"]["mean"]) < 1e-4 and abs(r["comp"] - want["comp"]["mean"]) < 1e-4


# --------------------------------------------------------------------------------------------------------- end to end
def _write_infer_folder(scan, sc):
    from PIL import Image
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(scan / sub, exist_ok=True)
    for i in range(sc["depths"].shape[0]):
        mvs_io.write_pfm(str(scan / "depth_est" / f"{i:08d}.pfm"), sc["depths"][i])
        mvs_io.write_pfm(str(scan / "confidence" / f"{i:08d}.pfm"), np.ascontiguousarray(sc["confs"][i].transpose(1, 2, 0)))
        mvs_io.write_cam_file(str(scan / "cams" / f"{i:08d}_cam.txt"), sc["cams"][i])
        Image.fromarray(sc["images"][i]).save(str(scan / "images" / f"{i:08d}.jpg"))


def test_filter_scan_reads_files_and_matches_restatement(tmp_path):
    sc = _synthetic(4, 40, 56, seed=9)
    scan = tmp_path / "scan3"
    _write_infer_folder(scan, sc)
    info = gipuma.filter_scan(str(scan), str(tmp_path / "scan3.ply"), prob_threshold=PROB, disp_threshold=0.4,
                              num_consistent=2)
    s = gipuma.load_scan(str(scan))                       # what is on disk (the JPEG colours, the cameras as text)
    want = R.fuse(list(s["depths"]), list(s["confs"]), list(s["cams"]), list(s["images"]), PROB, 0.4, 2)
    pts, col = fusion.read_ply(str(tmp_path / "scan3.ply"))
    assert info == {"points": want["points"].shape[0], "views": 4} and info["points"] > 0
    assert np.array_equal(pts.view(np.uint32), want["points"].view(np.uint32)) and np.array_equal(col, want["colors"])


def test_infer_fuse_gipuma_matches_cli(tmp_path):
    """infer --fuse --filter_method gipuma writes <out>/<scan>.ply; the CLI re-fuses the same folder to the same bytes."""
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanG", 4, 128, 160, seed=3)
    with open(tmp_path / "list.txt", "w") as f:
        f.write("scanG\n")
    out = str(tmp_path / "out")
    flags = ["--prob_threshold", "0.0,0.0,0.0", "--disp_threshold", "1.0", "--num_consistent", "1"]
    infer.main(["--testpath", root, "--testlist", str(tmp_path / "list.txt"), "--outdir", out, "--num_view", "3",
                "--max_h", "128", "--max_w", "160", "--interval_scale", "1.0", "--fuse", "--filter_method", "gipuma"] + flags)
    ply = os.path.join(out, "scanG.ply")
    first = open(ply, "rb").read()
    pts, col = fusion.read_ply(ply)
    assert pts.shape[0] > 0 and np.isfinite(pts).all()
    os.remove(ply)
    res = gipuma.main(["--outdir", out, "--testlist", str(tmp_path / "list.txt"), "--export_fusibile"] + flags)
    assert res["scanG"]["points"] == pts.shape[0] and res["scanG"]["views"] == 4
    assert open(ply, "rb").read() == first
    assert os.path.exists(os.path.join(out, "scanG", "points_mvsnet", "2333__00000003", "disp.dmb"))
