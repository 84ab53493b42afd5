"""DTU evaluation on the MI355X: the thinning and nearest-neighbour kernels against the numpy restatement of the MATLAB
code (tests/dtu_eval_ref.py), determinism, streams, the infer -> fuse -> evaluate chain and a DTU-scale scan."""
import json
import os
import time

import numpy as np
import pytest
import torch

import dtu_eval_ref as R
from cds_mvsnet_amd import dtu_eval, fusion, mvs_io, pointcloud, synth
from test_dtu_eval_cpu import _dtu_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


# ------------------------------------------------------------------------------------------------------------ thinning
def _thin_cases():
    rs = np.random.RandomState(11)
    clusters = np.concatenate([c + rs.randn(300, 3) * 0.05 for c in rs.uniform(-2, 2, (6, 3))])   # hundreds of neighbours
    dups = np.repeat(rs.uniform(-1, 1, (40, 3)), 5, 0)                                          # exact duplicates
    mixed = np.concatenate([clusters, dups, rs.uniform(-3, 3, (800, 3)), rs.uniform(-3, 3, (20, 3)) * 1e3])
    one_cell = rs.uniform(0, 0.05, (200, 3)) + 7.0                                              # all in one cell
    surface = synth.make_dtu_scene(3, 2, 0.05, 1.0, 1.0)["stl"]
    surface = surface + rs.randn(*surface.shape).astype(np.float32) * 0.03
    return {"clusters": (clusters, 0.2), "duplicates": (dups, 0.2), "mixed": (mixed, 0.2), "one_cell": (one_cell, 0.2),
            "surface": (surface, 0.2), "one": (np.array([[1.0, 2.0, 3.0]]), 0.2), "tiny_dst": (dups + 1e-3 * rs.randn(*dups.shape), 1e-3)}


@pytest.mark.parametrize("case", ["clusters", "duplicates", "mixed", "one_cell", "surface", "one", "tiny_dst"])
def test_reduce_points_matches_sequential_greedy(case):
    pts, dst = _thin_cases()[case]
    pts = np.asarray(pts, np.float32)
    order = pointcloud.thinning_order(len(pts), seed=1)
    want = R.reduce_pts(pts, dst, order.numpy())
    got = pointcloud.reduce_points(_g(pts), dst, order=order)
    assert got.dtype == torch.bool and got.device.type == "cuda"
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (case, int((got.cpu() != torch.from_numpy(want)).sum()))
    if case == "duplicates":                                 # of five copies at most one stays
        assert int(got.view(40, 5).sum(1).max()) == 1


def test_reduce_points_empty_seed_and_order():
    assert pointcloud.reduce_points(torch.zeros(0, 3, device=DEV), 0.2).numel() == 0
    pts, dst = _thin_cases()["mixed"]
    p = _g(pts)
    a = pointcloud.reduce_points(p, dst, seed=3)
    b = pointcloud.reduce_points(p, dst, order=pointcloud.thinning_order(len(pts), 3))
    assert torch.equal(a, b) and torch.equal(a, pointcloud.reduce_points(p, dst, seed=3))
    assert torch.equal(a.cpu(), torch.from_numpy(R.reduce_pts(pts, dst, pointcloud.thinning_order(len(pts), 3).numpy())))
    with pytest.raises(ValueError):
        pointcloud.reduce_points(p, dst, order=torch.zeros(len(pts), dtype=torch.long))
    with pytest.raises(ValueError):
        pointcloud.reduce_points(p, 0.0)


# ---------------------------------------------------------------------------------------------------- nearest distance
def _ulp_close(got, want, ulps=2):
    got = np.asarray(got, np.float32)
    want = np.asarray(want, np.float32)
    tol = ulps * np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))
    return np.abs(got - want) <= tol


def _nn_check(q, t, cap):
    got = pointcloud.nearest_distance(_g(q), _g(t), cap).cpu().numpy()
    want = np.minimum(R.brute_nn(q, t), np.float32(cap))
    ok = _ulp_close(got, want)
    assert ok.all(), (int((~ok).sum()), got[~ok][:5], want[~ok][:5])
    return got


@pytest.mark.parametrize("m,n", [(1, 1), (1, 5000), (5000, 1), (200_000, 3000), (3000, 200_000), (40_000, 40_000)])
def test_nearest_distance_sizes(m, n):
    rs = np.random.RandomState(m % 97 + n % 89)
    t = synth.make_dtu_scene(40, 30, 0.5, 2.0, 2.0)["stl"]
    t = t[rs.choice(len(t), n, replace=n > len(t))] + rs.randn(n, 3).astype(np.float32) * 0.2
    q = t[rs.choice(n, m)] + rs.randn(m, 3).astype(np.float32) * rs.choice([0.1, 2.0, 15.0], (m, 1)).astype(np.float32)
    _nn_check(q.astype(np.float32), t.astype(np.float32), 20.0)


def test_nearest_distance_special_cases():
    rs = np.random.RandomState(5)
    t = (rs.uniform(-1, 1, (3000, 3)) * np.array([5e3, 5e3, 1e3]) - 2e3).astype(np.float32)    # negative, 10^4 mm box
    q = np.concatenate([t[:100], t[100:300] + rs.randn(200, 3).astype(np.float32) * 30,            # duplicates: distance 0
                        rs.uniform(-1, 1, (200, 3)).astype(np.float32) * 2e4,                     # far outside
                        np.array([[1e6, -1e6, 3e5]], np.float32)]).astype(np.float32)
    got = _nn_check(q, t, 60.0)
    assert (got[:100] == 0).all() and (got == 60.0).any()
    _nn_check(q, t, 1e9)                                                                           # effectively uncapped
    empty = pointcloud.nearest_distance(_g(q), torch.zeros(0, 3, device=DEV), 7.5)
    assert empty.shape == (len(q),) and (empty == 7.5).all()
    assert pointcloud.nearest_distance(torch.zeros(0, 3, device=DEV), _g(t), 7.5).numel() == 0
    one = _g(np.array([[1.0, -2.0, 3.0]]))
    assert float(pointcloud.nearest_distance(one, one, 5.0)[0]) == 0.0


def test_nearest_distance_coarse_cell_choice_does_not_change_results():
    rs = np.random.RandomState(8)
    t = rs.uniform(-50, 50, (20_000, 3)).astype(np.float32)
    q = rs.uniform(-80, 80, (5000, 3)).astype(np.float32)
    want = np.minimum(R.brute_nn(q, t), np.float32(30.0))
    for cell in (0.05, 0.7, 3.0, 40.0):
        got = pointcloud.nearest_distance(_g(q), _g(t), 30.0, cell=cell).cpu().numpy()
        assert _ulp_close(got, want).all(), cell


def test_determinism_and_side_stream():
    rs = np.random.RandomState(9)
    pts, dst = _thin_cases()["surface"]
    p = _g(pts)
    q = _g(pts[rs.choice(len(pts), 20_000)] + rs.randn(20_000, 3).astype(np.float32))
    k1 = pointcloud.reduce_points(p, dst, seed=2)
    d1 = pointcloud.nearest_distance(q, p, 20.0)
    assert torch.equal(k1, pointcloud.reduce_points(p, dst, seed=2))
    assert torch.equal(d1, pointcloud.nearest_distance(q, p, 20.0))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        k2 = pointcloud.reduce_points(p, dst, seed=2)
        d2 = pointcloud.nearest_distance(q, p, 20.0)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(k1, k2) and torch.equal(d1, d2)


# ----------------------------------------------------------------------------------------------------------- end to end
def _assert_stats(got, want):
    for side in ("acc", "comp"):
        w = want[side]
        assert got[f"{side}_n"] == w["n"], side
        for k, gk in (("mean", side), ("median", f"{side}_median"), ("var", f"{side}_var")):
            assert abs(got[gk] - w[k]) <= 1e-6 * abs(w[k]), (side, k, got[gk], w[k])


def test_fuse_then_evaluate_cli_matches_oracle(tmp_path, capsys):
    """synthetic fusion scene -> fusion.filter_depth -> PLY -> the CLI on a DTU-layout folder; JSON vs the oracle."""
    from PIL import Image
    n, h, w = 4, 48, 64
    sc = synth.make_fusion_scene(n, h, w, seed=5, outlier_frac=0.05)
    scan = tmp_path / "out" / "scan9"
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(scan / sub)
    for i in range(n):
        mvs_io.write_pfm(str(scan / "depth_est" / f"{i:08d}.pfm"), sc["depths"][i].numpy())
        mvs_io.write_pfm(str(scan / "confidence" / f"{i:08d}.pfm"), np.ascontiguousarray(sc["confs"][i].permute(1, 2, 0).numpy()))
        mvs_io.write_cam_file(str(scan / "cams" / f"{i:08d}_cam.txt"), sc["cams"][i].numpy())
        Image.fromarray((sc["imgs"][i].numpy() * 255).astype(np.uint8)).save(str(scan / "images" / f"{i:08d}.jpg"))
    pairs = tmp_path / "in" / "scan9"
    os.makedirs(pairs)
    with open(pairs / "pair.txt", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            others = [j for j in range(n) if j != i]
            f.write(f"{i}\n{len(others)} " + " ".join(f"{j} 1.0" for j in others) + "\n")
    plydir = tmp_path / "out"
    info = fusion.filter_depth(str(pairs), str(scan), str(plydir / "scan9.ply"), conf=(0.1, 0.1, 0.1), thres_disp=1.0,
                               thres_view=2)
    assert info["points"] > 2000
    # one pixel is ~11 world units: thin at 5, count distances below 40, STL every 3 units, mask voxels of 8
    gt = synth.make_dtu_scene(330, 250, 3.0, 8.0, 20.0, plane_z=640.0)
    data = tmp_path / "MVS Data"
    _dtu_layout(data, 9, gt)
    out_json = tmp_path / "res.json"
    res = dtu_eval.main(["--datapath", str(data), "--plydir", str(plydir), "--scans", "scan9", "--dst", "5", "--max-dist", "40",
                         "--seed", "4", "--json", str(out_json)])
    printed = capsys.readouterr().out
    assert "scan9: acc" in printed and "mean over 1 scans" in printed
    j = json.load(open(out_json))
    pred = pointcloud.read_ply_points(str(plydir / "scan9.ply"))
    want = R.point_compare(pred, dtu_eval.load_dtu_scan(str(data), 9), 5.0, pointcloud.thinning_order(len(pred), 4).numpy(),
                           max_dist=40.0, block=120.0)
    got = j["scans"]["scan9"]
    assert got["n_thinned"] == int(want["keep"].sum()) and got["n_in_mask"] == int(want["data_in_mask"].sum())
    assert got["n_above_plane"] == int(want["stl_above_plane"].sum())
    _assert_stats(got, want)
    assert 0 < want["acc"]["n"] < got["n_thinned"] and 0 < want["comp"]["n"] < got["n_stl"]
    assert abs(j["mean"]["overall"] - (want["acc"]["mean"] + want["comp"]["mean"]) / 2) <= 1e-6 * want["overall"]
    assert res["mean"]["acc"] == got["acc"]


def test_evaluate_arrays_match_oracle_on_dtu_like_scene():
    sc = synth.make_dtu_scene(20, 15, 0.2, 0.5, 2.0, plane_z=655.0, n_pred=30_000, noise=0.15, outlier_frac=0.02,
                              outlier_range=30.0, holes=3, hole_radius=2.0, seed=3)
    r = dtu_eval.evaluate(_g(sc["pred"]), sc, seed=7, return_arrays=True)
    want = R.point_compare(sc["pred"], sc, 0.2, pointcloud.thinning_order(len(sc["pred"]), 7).numpy())
    assert torch.equal(r["keep"].cpu(), torch.from_numpy(want["keep"]))
    assert torch.equal(r["data_in_mask"].cpu(), torch.from_numpy(want["data_in_mask"]))
    assert torch.equal(r["stl_above_plane"].cpu(), torch.from_numpy(want["stl_above_plane"]))
    dd = want["ddata"][want["data_in_mask"]]
    ok = _ulp_close(r["ddata"].cpu().numpy(), np.minimum(dd, 20.0).astype(np.float32))
    assert ok.all()
    ds = want["dstl"][want["stl_above_plane"]]
    assert _ulp_close(r["dstl"].cpu().numpy(), np.minimum(ds, 20.0).astype(np.float32)).all()
    _assert_stats(r, want)


# --------------------------------------------------------------------------------------------------------------- DTU scale
def test_dtu_scale_scan():
    """~2.5 M STL points at 0.2 mm and ~25 M predicted points with noise, holes and outliers, at the protocol's 0.2 / 20."""
    t0 = time.time()
    sc = synth.make_dtu_scene(158, 158, 0.2, 2.0, 10.0, n_pred=26_000_000, noise=0.12, outlier_frac=0.01, outlier_range=25.0,
                              holes=6, hole_radius=8.0, seed=21)
    t_gen = time.time() - t0
    assert 2.3e6 < len(sc["stl"]) < 2.7e6 and len(sc["pred"]) > 2e7
    pred = _g(sc["pred"])
    torch.cuda.synchronize()
    timings = {}
    t1 = time.time()
    r = dtu_eval.evaluate(pred, sc, return_arrays=True, timings=timings)
    t_wall = time.time() - t1
    print(f"\nDTU-scale scan: {len(sc['pred'])} predicted, {len(sc['stl'])} STL points (generated in {t_gen:.1f} s); "
          f"acc {r['acc']:.4f} comp {r['comp']:.4f} overall {r['overall']:.4f}; thinned {r['n_thinned']}, "
          f"wall {t_wall:.2f} s")
    print("phases (ms): " + ", ".join(f"{k} {v:.1f}" for k, v in timings.items()))
    assert 0.05 < r["acc"] < 1.0 and 0.05 < r["comp"] < 5.0
    rs = np.random.RandomState(0)
    stl = _g(sc["stl"])
    # 500 sampled queries of each direction against brute force
    for q_all, target, d_all in ((r["data"][r["data_in_mask"]], stl, r["ddata"]), (stl[r["stl_above_plane"]], r["data"], r["dstl"])):
        idx = torch.from_numpy(rs.choice(q_all.shape[0], 250, replace=False)).to(DEV)
        q = q_all[idx]
        best = torch.full((q.shape[0],), float("inf"), device=DEV)
        for s in range(0, target.shape[0], 1 << 20):
            t = target[s:s + (1 << 20)]
            dx = t[None, :, 0] - q[:, None, 0]
            dy = t[None, :, 1] - q[:, None, 1]
            dz = t[None, :, 2] - q[:, None, 2]
            best = torch.minimum(best, (dx * dx + dy * dy + dz * dz).min(1)[0])
        want = torch.clamp(torch.sqrt(best), max=20.0).cpu().numpy()
        assert _ulp_close(d_all[idx].cpu().numpy(), want).all()
    # 200 sampled points against the thinning invariants
    order = pointcloud.thinning_order(pred.shape[0], 0).to(DEV)
    rank = torch.empty(pred.shape[0], dtype=torch.long, device=DEV)
    rank[order] = torch.arange(pred.shape[0], device=DEV)
    keep = r["keep"]
    dst2 = np.float32(0.2) * np.float32(0.2)
    for i in rs.choice(pred.shape[0], 200, replace=False):
        p = pred[i]
        d = pred - p
        near = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) <= float(dst2)
        near[i] = False
        if keep[i]:
            assert not bool((near & keep).any())
        else:
            assert bool((near & keep & (rank < rank[i])).any())
