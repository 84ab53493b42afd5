"""Dynamic-consistency fusion on the MI355X: cds_depth_fusion_dynamic_f32 against the float32 restatement
(tests/fusion_dynamic_ref.py) on the five test scenes, its optional outputs, view order, parameter monotonicity, the file
harness with its command line, and infer --fuse --filter_method dynamic.

Thresholded outputs (levels, admit, mask) may flip where a pixel sits on a threshold and the kernel's fp32 operation order
differs from torch's: the caps are those of tests/test_fusion.py (2e-3 per-view, 3e-3 per-pixel); the float32 and float64
restatements themselves differ in at most 3.3e-4 of the levels on these scenes (tests/test_fusion_dynamic_cpu.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fusion_dynamic_ref as R
from cds_mvsnet_amd import fusion, infer, mvs_io, synth
from test_mvs_io import _write_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(i, n_views=R.N_VIEWS, scale=1.0, want=True, order=None):
    V, h, w, seed, amp, conf = R.CASES[i]
    sc = R.make_case(V, h, w, seed, amp)
    src = list(range(1, V + 1)) if order is None else order
    return fusion.fuse_view_dynamic(sc["depths"][0].cuda(), sc["confs"][0].cuda(), sc["cams"][0], sc["depths"][src].cuda(),
                                    sc["confs"][src].cuda(), sc["cams"][src], conf=conf, dist_base=R.DIST_BASE * scale,
                                    rel_base=R.REL_BASE * scale, n_views=n_views, want_admit=want, want_levels=want)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_kernel_vs_reference(i):
    V, h, w = R.CASES[i][:3]
    exp = R.case_reference(i)
    out = _run(i)
    assert out["levels"].dtype == torch.uint8 and out["admit"].dtype == torch.uint8
    assert tuple(out["levels"].shape) == (V, h, w) and tuple(out["admit"].shape) == (h, w)
    levels, admit, mask = out["levels"].cpu().long(), out["admit"].cpu().long(), out["mask"].cpu()
    lv = (levels != exp["levels"]).float().mean().item()
    mk = (mask != exp["mask"]).float().mean().item()
    ad = (admit != exp["admit"]).float().mean().item()
    same = (levels == exp["levels"]).all(0)
    dd = (out["depth"].cpu() - exp["depth"]).abs()[same].max().item()
    dp = (out["points"].cpu() - exp["points"]).abs()[:, same].max().item()
    print(f"{R.CASE_IDS[i]}: levels {lv:.2e}, mask {mk:.2e}, admit {ad:.2e}, depth {dd:.2e}, points {dp:.2e}, "
          f"kept {mask.mean().item():.3f}")
    assert set(mask.unique().tolist()) <= {0.0, 1.0} and int(levels.min()) >= 1 and int(levels.max()) <= R.N_VIEWS[1] + 1
    assert lv < 2e-3
    assert mk < 3e-3 and ad < 3e-3
    assert dd < 2e-2 and dp < 2e-2                       # depths ~650 (3e-5 relative)
    if V == 1:                                           # V < n_min admits nothing
        sc = R.make_case(*R.CASES[i][:5])
        assert mask.sum().item() == 0 and admit.sum().item() == 0
        bad = levels[0] == R.N_VIEWS[1] + 1
        assert bad.any() and torch.equal(out["depth"].cpu()[bad], sc["depths"][0][bad])


def test_optional_outputs_do_not_change_the_rest():
    a, b = _run(2, want=True), _run(2, want=False)
    assert "admit" not in b and "levels" not in b
    for k in ("depth", "mask", "points"):
        assert torch.equal(a[k], b[k]), k


def test_view_order():
    V = R.CASES[2][0]
    a, b = _run(2), _run(2, order=list(range(V, 0, -1)))
    assert torch.equal(a["mask"], b["mask"]) and torch.equal(a["admit"], b["admit"])
    assert torch.equal(a["levels"], b["levels"].flip(0))
    assert (a["depth"] - b["depth"]).abs().max().item() < 2e-2      # the average runs in view order: fp32 summation order


def test_parameter_sanity():
    base = _run(3)["mask"] > 0.5
    tight = _run(3, n_views=(2, 2))["mask"] > 0.5
    loose = _run(3, scale=2.0)["mask"] > 0.5
    print(f"kept: (2,2) {tight.float().mean().item():.3f}, (2,10) {base.float().mean().item():.3f}, doubled bases "
          f"{loose.float().mean().item():.3f}")
    assert not (tight & ~base).any() and tight.sum() < base.sum()
    assert not (base & ~loose).any() and base.sum() < loose.sum()


def test_filter_depth_dynamic_harness(tmp_path):
    """Files in the layout infer writes -> fused PLY, through filter_depth and through the command line."""
    from PIL import Image
    n, h, w, conf = 4, 48, 64, (0.1, 0.1, 0.1)
    sc = synth.make_fusion_scene(n, h, w, seed=5, outlier_frac=0.05)
    scan = tmp_path / "out" / "scan1"
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(scan / sub)
    for i in range(n):
        mvs_io.write_pfm(str(scan / "depth_est" / f"{i:08d}.pfm"), sc["depths"][i].numpy())
        mvs_io.write_pfm(str(scan / "confidence" / f"{i:08d}.pfm"), np.ascontiguousarray(sc["confs"][i].permute(1, 2, 0).numpy()))
        mvs_io.write_cam_file(str(scan / "cams" / f"{i:08d}_cam.txt"), sc["cams"][i].numpy())
        Image.fromarray((sc["imgs"][i].numpy() * 255).astype(np.uint8)).save(str(scan / "images" / f"{i:08d}.jpg"))
    pairs = tmp_path / "in" / "scan1"
    os.makedirs(pairs)
    with open(pairs / "pair.txt", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            others = [j for j in range(n) if j != i]
            f.write(f"{i}\n{len(others)} " + " ".join(f"{j} 1.0" for j in others) + "\n")
    ply = str(tmp_path / "out" / "scan1.ply")
    info = fusion.filter_depth(str(pairs), str(scan), ply, conf=conf, method="dynamic")
    first = open(ply, "rb").read()
    pts, col = fusion.read_ply(ply)
    assert pts.shape[0] == info["points"] and col.shape == pts.shape and np.isfinite(pts).all()
    n_exp, geo, geo_exp = 0, [], []
    for i in range(n):
        others = [j for j in range(n) if j != i]
        cams = torch.stack([torch.from_numpy(fusion.read_fusion_cam(str(scan / "cams" / f"{j:08d}_cam.txt"))) for j in [i] + others])
        e = R.fuse_view_dynamic(sc["depths"][i], sc["confs"][i], cams[0], sc["depths"][others], sc["confs"][others], cams[1:],
                                conf=conf)
        n_exp += int(e["mask"].sum())
        geo_exp.append((e["admit"] > 0).float().mean().item())
        o = fusion.fuse_view_dynamic(sc["depths"][i].cuda(), sc["confs"][i].cuda(), cams[0], sc["depths"][others].cuda(),
                                     sc["confs"][others].cuda(), cams[1:], conf=conf, want_admit=True)
        geo.append((o["admit"] > 0).float().mean().item())
    print(f"points {pts.shape[0]} (reference {n_exp}), admitted at {info['admitted_at']}, geometric share {np.mean(geo):.4f} "
          f"(reference {np.mean(geo_exp):.4f})")
    assert abs(pts.shape[0] - n_exp) <= max(3, 0.003 * n_exp)
    assert n_exp > 100        # the restatement keeps 418 pixels: three source views admit at n <= 3 only, on a coarse grid
    assert sorted(info["admitted_at"]) == list(range(2, 11))
    assert abs(sum(info["admitted_at"].values()) - np.mean(geo)) < 1e-6       # the shares sum to the geometric share
    assert abs(np.mean(geo) - np.mean(geo_exp)) <= 0.003                      # the admit cap of the kernel test
    assert sum(info["admitted_at"].values()) + 1e-9 >= info["mean_final_mask"]
    assert np.median(np.abs(pts[:, 2] - synth.fusion_surface(pts[:, 0], pts[:, 1]))) < 2.0
    # the command line, as a child process, writes the same bytes
    os.remove(ply)
    with open(tmp_path / "list.txt", "w") as f:
        f.write("scan1\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "cds_mvsnet_amd.fusion", "--testpath", str(tmp_path / "in"), "--outdir",
                          str(tmp_path / "out"), "--testlist", str(tmp_path / "list.txt"), "--filter_method", "dynamic",
                          "--conf", "0.1,0.1,0.1"], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert f"scan1.ply: {info['points']} points" in res.stdout and "admitted at n=" in res.stdout
    assert open(ply, "rb").read() == first
    # the default method is untouched: today's keys
    normal = fusion.filter_depth(str(pairs), str(scan), str(tmp_path / "normal.ply"), conf=conf, thres_view=2)
    assert set(normal) == {"points", "mean_final_mask"}


def test_infer_fuse_dynamic(tmp_path, capsys):
    """infer --fuse --filter_method dynamic on the tiny synthetic scan of test_inference_harness_end_to_end.  The network is
    untrained, so its depth maps agree only loosely: one agreeing view is enough here and the bases are wide."""
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanA", 4, 128, 160, seed=3)
    with open(tmp_path / "list.txt", "w") as f:
        f.write("scanA\n")
    out = str(tmp_path / "out")
    infer.main(["--testpath", root, "--testlist", str(tmp_path / "list.txt"), "--outdir", out, "--num_view", "3",
                "--max_h", "128", "--max_w", "160", "--interval_scale", "1.0", "--fuse", "--filter_method", "dynamic",
                "--conf", "0.0,0.0,0.0", "--dyn_dist_base", "2.0", "--dyn_rel_base", "0.02", "--dyn_views", "1,10"])
    pts, col = fusion.read_ply(os.path.join(out, "scanA.ply"))
    assert pts.shape[0] > 0 and pts.shape == col.shape and np.isfinite(pts).all()
    line = [ln for ln in capsys.readouterr().out.splitlines() if "scanA.ply" in ln]
    assert line and f"{pts.shape[0]} points" in line[0] and "admitted at" in line[0] and "(dynamic)" in line[0]
