"""Outlier removal for fused clouds on the MI355X: cds_knn_mean_f64, cds_radius_count_f32 and
cds_outlier_stats_f64 against the numpy restatement of tests/cloud_outlier_ref.py, pointcloud.remove_outliers on a planted
case, and the way through filter_depth, gipuma and the command line.

Bounds.  Every rule is a function of the inputs with a stated order of operations, and the device's sqrt and divide are
correctly rounded, so means, k-th distances, mu, sigma and the masks must be equal to the bit; counts are integers.

Shapes.  Point counts around k and around the 256-lane workgroup, one larger cloud with several workgroups; a cloud inside one
fine cell, the same cloud in a grid of ~100 fine cells per axis (13 coarse cells: almost everything is found by the ring walk,
and an unfilled list walks a grid small enough to exhaust; up to 257 points nearly every point is alone in its coarse cell),
the 1500 points also in a grid of ~500 fine cells per axis with the finite caps (63^3 coarse cells: but for a handful of pairs
every point alone in its coarse cell, everything found by the ring walk; a list that stays unfilled walks as many coarse
cells as its cap reaches, up to 250 000, which an infinite cap or the large caps of the small clouds make every query do:
measured, 13 s for the k = 64 case instead of 1), an integer lattice (ties at the k-th place), exact duplicates,
queries off the cloud and outside the grid's box."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_outlier_ref as R
import tt_eval_ref
from cds_mvsnet_amd import _lib, fusion, gipuma, mvs_io, pointcloud, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 2, 21, 64]
CONF = (0.1, 0.1, 0.1)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _cloud(n, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def _queries(cloud, seed):
    """The cloud itself, points near it that are not in it, and a few outside its bounding box (some far outside)."""
    rs = np.random.RandomState(seed)
    off = rs.uniform(-1.0, 1.0, (12, 3))
    outside = np.array([[1.5, 0, 0], [-3.0, 0.2, 0.1], [0.3, 4.0, -0.2], [2.0, 2.0, 2.0], [0, 0, -1.2]])
    return np.concatenate([cloud, off.astype(np.float32), outside.astype(np.float32)])


def _caps(query, cloud, k):
    """inf, a value that cuts about half the lists (the median k-th distance), a value below every non-zero distance."""
    d2 = np.sort(R.pair_d2(query, cloud), axis=1)
    kth = np.sqrt(d2[:, min(k, d2.shape[1]) - 1])
    nz = d2[d2 > 0]
    low = 0.5 * float(np.sqrt(nz.min())) if nz.size else 0.5
    return [np.inf, float(np.median(kth)) if float(np.median(kth)) > 0 else 0.25, low]


def _check_knn(query, cloud, k, cell, what, finite_only=False):
    grid = pointcloud.PointGrid(_dev(cloud), cell)
    q = _dev(query)
    for cap in _caps(query, cloud, k)[1 if finite_only else 0:]:
        want_mean, want_kth = R.knn_mean(query, cloud, k, cap)
        mean, kth = pointcloud.knn_mean_distance(q, None, k, cap, grid=grid, want_kth=True)
        assert mean.dtype == torch.float64 and kth.dtype == torch.float32
        mean, kth = mean.cpu().numpy(), kth.cpu().numpy()
        capped = int((want_kth == np.float32(cap)).sum())
        bad_m, bad_k = int((_bits(mean) != _bits(want_mean)).sum()), int((_bits(kth) != _bits(want_kth)).sum())
        print(f"{what} k={k} cap={cap:.4g}: {len(query)} queries, {capped} with a capped term, mean differs in {bad_m}, "
              f"kth in {bad_k}")
        assert bad_m == 0 and bad_k == 0
        alone = pointcloud.knn_mean_distance(q, None, k, cap, grid=grid)
        assert torch.equal(alone.cpu(), torch.from_numpy(mean))


@pytest.mark.parametrize("k", KS)
def test_knn_mean_point_counts_and_cells(k):
    for n in sorted({1, 2, max(k - 1, 1), k, k + 1, 255, 256, 257, 1500}):
        cloud = _cloud(n, 10 * n + k)
        query = _queries(cloud, n)
        ext = max(float((cloud.max(0) - cloud.min(0)).max()), 1e-3)
        _check_knn(query, cloud, k, 10.0 * ext, f"n={n} one cell")
        _check_knn(query, cloud, k, ext / 100.0, f"n={n} tiny cells")
        if n == 1500:
            _check_knn(query, cloud, k, ext / 500.0, f"n={n} own coarse cells", finite_only=True)


@pytest.mark.parametrize("k", KS)
def test_knn_mean_lattice_and_duplicates(k):
    g = np.arange(6, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    query = np.concatenate([lattice, lattice[:20] + np.float32(0.5), [[-2.0, 2.5, 9.0]]]).astype(np.float32)
    grid = pointcloud.PointGrid(_dev(lattice), 1.0)
    for cap in (np.inf, 2.0, 1.0, 0.5):               # 2 and 1 are lattice distances: d2 < cap^2 is strict
        want_mean, want_kth = R.knn_mean(query, lattice, k, cap)
        mean, kth = pointcloud.knn_mean_distance(_dev(query), None, k, cap, grid=grid, want_kth=True)
        assert np.array_equal(_bits(mean.cpu().numpy()), _bits(want_mean)), cap
        assert np.array_equal(_bits(kth.cpu().numpy()), _bits(want_kth)), cap
    rs = np.random.RandomState(k)
    base = _cloud(700, 77)
    cloud = np.concatenate([base, base[rs.randint(0, 700, 300)]])[rs.permutation(1000)]       # 30 % exact duplicates
    _check_knn(_queries(cloud, 5), cloud, k, pointcloud.default_cell(_dev(cloud)), "duplicates")


def test_knn_mean_default_grid_and_workgroup_sizes():
    cloud = _cloud(1500, 3)
    want = R.knn_mean(cloud, cloud, 21, 0.3)[0]
    d = _dev(cloud)
    assert np.array_equal(_bits(pointcloud.knn_mean_distance(d, d, 21, 0.3).cpu().numpy()), _bits(want))
    # the entry point that takes the workgroup size: the same bits at every size, other sizes refused
    grid = pointcloud.PointGrid(d, pointcloud.default_cell(d))
    got = torch.empty(len(cloud), dtype=torch.float64, device="cuda")
    for threads, rc in ((64, 0), (128, 0), (256, 0), (0, _lib.EINVAL), (100, _lib.EINVAL), (512, _lib.EINVAL)):
        got.fill_(-1.0)
        assert _lib.load().cds_knn_mean_wg_f64(d.data_ptr(), None, len(cloud), *pointcloud._grid_args(grid), 21, 0.3, got.data_ptr(),
                                               None, threads, None) == rc, threads
        assert rc != 0 or np.array_equal(_bits(got.cpu().numpy()), _bits(want)), threads
    for k in (0, 65):
        with pytest.raises(ValueError):
            pointcloud.knn_mean_distance(_dev(cloud), _dev(cloud), k)
    with pytest.raises(ValueError):
        pointcloud.knn_mean_distance(_dev(cloud), _dev(cloud), 3, max_dist=-1.0)
    assert pointcloud.knn_mean_distance(_dev(cloud[:0]), _dev(cloud), 3).shape == (0,)


def test_every_sink_walks_the_same_grid():
    """One walk, three sinks (grid_common.hpp): over one index_grid and one query set, nearest_distance, the dist of
    nearest_index and the k-th distance of knn_mean_distance(k = 1) are the same bits, and nearest_index's index is that of
    tt_eval_ref (argmin of the fp32 d2, the lowest index among ties, -1 where d2 >= cap^2).  Shapes where a walk can go wrong:
    one target point, 257 points in one fine cell, 1500 points in ~100 fine cells per axis (the ring walk finds almost
    everything), the 6^3 lattice with cell 1 and caps that are lattice distances; queries on the cloud, off it and outside
    the grid's box."""
    cases = []
    for n, cells in ((1, 0.1), (257, 0.1), (1500, 100.0)):
        cloud = _cloud(n, 31 * n)
        query = _queries(cloud, n)
        ext = max(float((cloud.max(0) - cloud.min(0)).max()), 1e-3)
        cases.append((f"n={n}", cloud, query, ext / cells, _caps(query, cloud, 1)))
    g = np.arange(6, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    face = lattice[:36]                                # x = 0; moved out by 1 and 2: nearest at exactly a cap, not accepted
    query = np.concatenate([lattice, lattice + np.float32(0.5), face - np.float32([1, 0, 0]), face - np.float32([2, 0, 0])])
    cases.append(("lattice", lattice, query, 1.0, [1.0, 2.0, np.inf]))
    for name, cloud, query, cell, caps in cases:
        grid = pointcloud.index_grid(_dev(cloud), cell)
        q = _dev(query)
        for cap in caps:
            want_d, want_i = tt_eval_ref.nearest_index(query, cloud, cap)
            alone = pointcloud.nearest_distance(q, _dev(cloud), cap, grid=grid).cpu().numpy()
            dist, index = pointcloud.nearest_index(q, _dev(cloud), cap, grid=grid)
            kth = pointcloud.knn_mean_distance(q, None, 1, cap, grid=grid, want_kth=True)[1].cpu().numpy()
            dist, index = dist.cpu().numpy(), index.cpu().numpy()
            print(f"{name} cap={cap:.4g}: {len(query)} queries, {int((index < 0).sum())} without a neighbour; differing from "
                  f"nearest_distance: nearest_index {int((_bits(dist) != _bits(alone)).sum())}, knn k=1 "
                  f"{int((_bits(kth) != _bits(alone)).sum())}; index differs in {int((index != want_i).sum())}")
            assert alone.dtype == dist.dtype == kth.dtype == np.float32 and index.dtype == np.int32
            assert np.array_equal(_bits(dist), _bits(alone)), (name, cap)
            assert np.array_equal(_bits(kth), _bits(alone)), (name, cap)
            assert np.array_equal(index, want_i), (name, cap)
            assert np.array_equal(_bits(dist), _bits(want_d)), (name, cap)


def test_radius_count():
    g = np.arange(6, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    cases = [("lattice", lattice, np.concatenate([lattice, lattice[:20] + np.float32(0.5), [[-2.0, 2.5, 9.0]]]).astype(np.float32),
              [1.0, 2.0, float(np.sqrt(np.float32(2.0))), 0.4])]
    for n in (1, 2, 257, 1500):
        c = _cloud(n, n)
        cases.append((f"n={n}", c, _queries(c, n), [0.05, 0.3, 2.5]))
    base = _cloud(700, 77)
    rs = np.random.RandomState(1)
    dup = np.concatenate([base, base[rs.randint(0, 700, 300)]])[rs.permutation(1000)]
    cases.append(("duplicates", dup, _queries(dup, 5), [0.05, 0.3]))
    for name, cloud, query, radii in cases:
        for radius in radii:
            full = R.radius_count(query, cloud, radius, 10 ** 9)
            for cap in (1, 7, len(cloud) + 5):
                got = pointcloud.radius_count(_dev(query), _dev(cloud), radius, cap).cpu().numpy()
                assert got.dtype == np.int32 and np.array_equal(got, np.minimum(full, cap)), (name, radius, cap)
            print(f"{name} r={radius:.3g}: counts {full.min()}..{full.max()}")
    # a supplied grid: fine when its cell covers the radius, refused when it does not
    grid = pointcloud.PointGrid(_dev(lattice), 1.5)
    assert np.array_equal(pointcloud.radius_count(_dev(lattice), None, 1.0, 99, grid=grid).cpu().numpy(),
                          R.radius_count(lattice, lattice, 1.0, 99))
    with pytest.raises(ValueError, match="cell"):
        pointcloud.radius_count(_dev(lattice), None, 2.0, 99, grid=grid)
    f = grid.frame
    out = torch.zeros(len(lattice), dtype=torch.int32, device="cuda")
    rc = _lib.load().cds_radius_count_f32(_dev(lattice).data_ptr(), None, len(lattice), grid.pts.data_ptr(), grid.cell_start.data_ptr(),
                                          grid.cell_keys.data_ptr(), grid.coarse_start.data_ptr(), grid.table_keys.data_ptr(),
                                          grid.table_vals.data_ptr(), grid.log2_slots, f.data_ptr(), 2.0, 99, out.data_ptr(), None)
    assert rc == _lib.EINVAL
    with pytest.raises(ValueError):
        pointcloud.radius_count(_dev(lattice), _dev(lattice), 0.0, 3)
    with pytest.raises(ValueError):
        pointcloud.radius_count(_dev(lattice), _dev(lattice), 1.0, 0)


@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 20000])
def test_outlier_stats(n):
    rs = np.random.RandomState(n)
    x = np.abs(rs.randn(n)) * 10.0 ** rs.uniform(-3, 3, n)
    mu, sigma = R.stats(x)
    got = pointcloud.outlier_stats(_dev(x)).cpu().numpy()
    print(f"n={n}: mu {got[0]!r} (want {float(mu)!r}), sigma {got[1]!r} (want {float(sigma)!r})")
    assert got.dtype == np.float64
    assert _bits(got).tolist() == _bits(np.array([mu, sigma], np.float64)).tolist()


# --------------------------------------------------------------------------------------------------------- the planted case
@functools.lru_cache(maxsize=None)
def _planted(seed):
    pts, is_out = R.planted_sphere(seed)
    ref = {key: R.remove_outliers(pts, **dict(key)) for key in (
        (("nb_neighbors", 20), ("std_ratio", 2.0)), (("nb_neighbors", 8), ("std_ratio", 1.0)),
        (("radius", 0.2), ("min_neighbors", 6)))}
    return pts, is_out, ref


def _mask(pts, **kw):
    info = {}
    keep = pointcloud.remove_outliers(_dev(pts), info=info, **kw)
    assert keep.dtype == torch.bool and keep.is_cuda
    return keep.cpu().numpy(), info


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_remove_outliers_planted_sphere(seed):
    pts, is_out, ref = _planted(seed)
    for key, least in (((("nb_neighbors", 20), ("std_ratio", 2.0)), 90), ((("nb_neighbors", 8), ("std_ratio", 1.0)), 100)):
        want, winfo = ref[key]
        gap = float(np.abs(winfo["mean"] - winfo["threshold"]).min() / winfo["threshold"])
        keep, info = _mask(pts, **dict(key))
        removed_out, removed_in = int((~keep & is_out).sum()), int((~keep & ~is_out).sum())
        print(f"seed {seed} {dict(key)}: outliers removed {removed_out}, inliers removed {removed_in}, threshold "
              f"{info['threshold']!r}, nearest relative gap {gap:.2e}")
        assert gap > 1e-9                                    # no m_i at the threshold: exact masks are a fair demand
        assert np.array_equal(keep, want)
        assert (info["mu"], info["sigma"], info["threshold"]) == (winfo["mu"], winfo["sigma"], winfo["threshold"])
        assert info["removed_statistical"] == winfo["removed_statistical"] and info["removed_radius"] == 0
        assert removed_in == 0 and removed_out >= least
    want, winfo = ref[(("radius", 0.2), ("min_neighbors", 6))]
    keep, info = _mask(pts, radius=0.2, min_neighbors=6)
    assert np.array_equal(keep, want) and np.array_equal(keep, ~is_out)
    assert info["removed_radius"] == 100 and info["removed_statistical"] == 0 and info["threshold"] is None
    # both filters: each judged on the input cloud
    both, info = _mask(pts, nb_neighbors=20, std_ratio=2.0, radius=0.2, min_neighbors=6)
    assert np.array_equal(both, ref[(("nb_neighbors", 20), ("std_ratio", 2.0))][0] & want)
    assert info["removed_radius"] == 100 and info["removed_statistical"] >= 90


def test_order_bits_and_small_clouds():
    pts, _, _ = _planted(0)
    d = _dev(pts)
    before = d.clone()
    keep = pointcloud.remove_outliers(d, nb_neighbors=8, std_ratio=1.0)
    assert torch.equal(d, before)                                             # the input is read only
    assert np.array_equal(d[keep].cpu().numpy().view(np.uint32), pts[keep.cpu().numpy()].view(np.uint32))
    assert torch.equal(pointcloud.remove_outliers(d, nb_neighbors=8, std_ratio=1.0), keep)
    assert pointcloud.remove_outliers(d, nb_neighbors=0).all()               # nothing asked for, nothing removed
    assert pointcloud.remove_outliers(d[:0], nb_neighbors=8).shape == (0,)
    assert pointcloud.remove_outliers(d[:1], nb_neighbors=8, radius=0.1, min_neighbors=0 + 1).tolist() == [False]
    assert pointcloud.remove_outliers(d[:1], nb_neighbors=8).tolist() == [True]
    same = torch.full((300, 3), 0.25, device="cuda")
    info = {}
    assert pointcloud.remove_outliers(same, nb_neighbors=5, std_ratio=0.0, info=info).all()   # m = T = 0: kept (<=)
    assert (info["mu"], info["sigma"], info["threshold"]) == (0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="nb_neighbors"):
        pointcloud.remove_outliers(d, nb_neighbors=64)
    with pytest.raises(ValueError, match="min_neighbors"):
        pointcloud.remove_outliers(d, radius=0.1)


# ------------------------------------------------------------------------------------------------------------- pipeline
def _write_outputs(tmp_path):
    from PIL import Image
    n, h, w = 3, 24, 40
    sc = synth.make_fusion_scene(n, h, w, outlier_frac=0.15)
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
    with open(tmp_path / "list.txt", "w") as f:
        f.write("scan1\n")
    return scan, pairs


def _by_hand(path, **kw):
    p, c, n = fusion.read_ply_full(path)
    info = {}
    keep = pointcloud.remove_outliers(_dev(p), info=info, **kw).cpu().numpy()
    return p[keep], c[keep], None if n is None else n[keep], info, len(p)


def _same_cloud(path, want):
    p, c, n = fusion.read_ply_full(path)
    assert np.array_equal(p.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(c, want[1])
    assert (n is None) == (want[2] is None) and (n is None or np.array_equal(n.view(np.uint32), want[2].view(np.uint32)))


def test_filter_depth_and_the_command_line(tmp_path):
    scan, pairs = _write_outputs(tmp_path)
    kw = dict(conf=CONF, thres_view=2)
    keys = {"mu", "sigma", "threshold", "removed_statistical", "removed_radius", "outliers_removed"}
    # without the flags: the keys and the bytes of before, twice
    plain = str(tmp_path / "plain.ply")
    info0 = fusion.filter_depth(str(pairs), str(scan), plain, **kw)
    assert set(info0) == {"points", "mean_final_mask"}
    first = open(plain, "rb").read()
    fusion.filter_depth(str(pairs), str(scan), plain, outlier_nb=0, outlier_radius=0.0, **kw)
    assert open(plain, "rb").read() == first
    for name, extra in (("alone", {}), ("merged", dict(merge_voxel=30.0)), ("normals", dict(normals=True))):
        base, cleaned = str(tmp_path / f"{name}0.ply"), str(tmp_path / f"{name}1.ply")
        fusion.filter_depth(str(pairs), str(scan), base, **extra, **kw)
        info = fusion.filter_depth(str(pairs), str(scan), cleaned, outlier_nb=8, **extra, **kw)
        p, c, n, hand, before = _by_hand(base, nb_neighbors=8)
        print(f"{name}: {before} points, {hand['removed_statistical']} removed, threshold {hand['threshold']!r}")
        _same_cloud(cleaned, (p, c, n))
        assert keys <= set(info) and info["points"] == len(p) and info["outliers_removed"] == before - len(p) > 0
        assert info["threshold"] == hand["threshold"] and (n is not None) == (name == "normals")
        if name == "merged":
            assert info["merged_from"] == info0["points"] > before
    # both filters through filter_depth; the radius: twice the median distance to the third other point
    p0 = fusion.read_ply_full(plain)[0]
    radius = 2.0 * float(np.median(R.knn_mean(p0, p0, 4)[1]))
    both = str(tmp_path / "both.ply")
    info = fusion.filter_depth(str(pairs), str(scan), both, outlier_nb=8, outlier_std=1.0, outlier_radius=radius, outlier_min_nb=3,
                               **kw)
    p, c, n, hand, before = _by_hand(plain, nb_neighbors=8, std_ratio=1.0, radius=radius, min_neighbors=3)
    print(f"both: {before} points, statistical {hand['removed_statistical']}, radius {radius:.4g} removes {hand['removed_radius']}")
    _same_cloud(both, (p, c, n))
    assert info["removed_radius"] == hand["removed_radius"] and info["removed_statistical"] == hand["removed_statistical"]
    assert 0 < len(p) < before
    with pytest.raises(ValueError, match="min_neighbors"):
        fusion.filter_depth(str(pairs), str(scan), both, outlier_radius=1.0, **kw)
    with pytest.raises(ValueError, match="plyfilename"):
        fusion.filter_depth(str(pairs), str(scan), None, collect=[], outlier_nb=8, **kw)
    with pytest.raises(ValueError, match="max_dist"):
        fusion.filter_depth(str(pairs), str(scan), both, outlier_max_dist=5.0, **kw)
    # fusion --from_ply in a child process: the saved cloud with normals, cleaned again
    src = str(tmp_path / "normals0.ply")
    out = tmp_path / "clean"
    os.makedirs(out)
    os.makedirs(tmp_path / "saved")
    os.replace(src, tmp_path / "saved" / "scan1.ply")
    src = str(tmp_path / "saved" / "scan1.ply")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "cds_mvsnet_amd.fusion", "--from_ply", str(tmp_path / "saved" / "{scan}.ply"), "--outdir",
                          str(out), "--testlist", str(tmp_path / "list.txt"), "--outlier_nb", "8"],
                         env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    p, c, n, hand, before = _by_hand(src, nb_neighbors=8)
    _same_cloud(str(out / "scan1.ply"), (p, c, n))
    assert f"scan1.ply: {len(p)} points, outliers removed {before - len(p)} (threshold " in res.stdout
    # the fusion command line itself
    res = fusion.main(["--testpath", str(tmp_path / "in"), "--outdir", str(tmp_path / "out"), "--testlist", str(tmp_path / "list.txt"),
                       "--conf", "0.1,0.1,0.1", "--thres_view", "2", "--outlier_nb", "8"])
    assert open(tmp_path / "out" / "scan1.ply", "rb").read() == open(tmp_path / "alone1.ply", "rb").read()
    assert res["scan1"]["outliers_removed"] > 0


def test_gipuma_filter_scan(tmp_path):
    scan, _ = _write_outputs(tmp_path)
    kw = dict(prob_threshold=CONF, disp_threshold=0.4, num_consistent=2)
    base, cleaned = str(tmp_path / "g0.ply"), str(tmp_path / "g1.ply")
    info0 = gipuma.filter_scan(str(scan), base, **kw)
    assert set(info0) == {"points", "views"}
    info = gipuma.filter_scan(str(scan), cleaned, outlier_nb=8, **kw)
    p, c, n, hand, before = _by_hand(base, nb_neighbors=8)
    _same_cloud(cleaned, (p, c, None))
    assert before == info0["points"] and info["points"] == len(p) and info["outliers_removed"] == before - len(p) > 0
    assert info["threshold"] == hand["threshold"] and info["views"] == 3
    # after the voxel merge when both are given
    gipuma.filter_scan(str(scan), str(tmp_path / "g2.ply"), merge_voxel=30.0, **kw)
    merged = gipuma.filter_scan(str(scan), str(tmp_path / "g3.ply"), merge_voxel=30.0, outlier_nb=8, **kw)
    p, c, n, hand, voxels = _by_hand(str(tmp_path / "g2.ply"), nb_neighbors=8)
    _same_cloud(str(tmp_path / "g3.ply"), (p, c, None))
    assert merged["merged_from"] == before > voxels == merged["points"] + merged["outliers_removed"]
