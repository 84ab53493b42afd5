"""Outlier removal for fused clouds without a GPU: the numpy restatement of tests/cloud_outlier_ref.py on cases
that can be checked by hand, the fixed summation order against scalar loops, the declarations, and the command lines."""
import os
import re

import numpy as np
import pytest

import cloud_outlier_ref as R
from cds_mvsnet_amd import _lib, fusion, gipuma, infer, pointcloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_IO = ["--testpath", "a", "--outdir", "b", "--testlist", "c"]
LINE = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [7, 0, 0]], np.float32)


def test_four_collinear_points():
    # k = 2: the point itself and its nearest other
    mean, kth = R.knn_mean(LINE, LINE, 2)
    assert mean.tolist() == [0.5, 0.5, 1.0, 2.0] and kth.tolist() == [1.0, 1.0, 2.0, 4.0]
    assert mean.dtype == np.float64 and kth.dtype == np.float32
    # a cap of 3: the last point's neighbour at 4 is beyond it and counts as 3; a distance equal to the cap is capped too
    mean, kth = R.knn_mean(LINE, LINE, 2, 3.0)
    assert mean.tolist() == [0.5, 0.5, 1.0, 1.5] and kth.tolist() == [1.0, 1.0, 2.0, 3.0]
    mean, kth = R.knn_mean(LINE, LINE, 2, 2.0)
    assert mean.tolist() == [0.5, 0.5, 1.0, 1.0] and kth.tolist() == [1.0, 1.0, 2.0, 2.0]
    # a query that is no grid point, every term capped
    mean, kth = R.knn_mean(np.array([[0, 100, 0]], np.float32), LINE, 3, 5.0)
    assert mean.tolist() == [5.0] and kth.tolist() == [5.0]
    # ascending order of the sum: (0 + 1) + 3 for the first point with k = 3
    assert R.knn_mean(LINE, LINE, 3)[0].tolist() == [4.0 / 3.0, 3.0 / 3.0, 5.0 / 3.0, 10.0 / 3.0]


def test_fewer_points_than_k():
    mean, kth = R.knn_mean(LINE, LINE, 6)                       # no cap: min(k, n) = 4 terms
    assert mean.tolist() == [11.0 / 4.0, 9.0 / 4.0, 9.0 / 4.0, 17.0 / 4.0] and kth.tolist() == [7.0, 6.0, 4.0, 7.0]
    mean, kth = R.knn_mean(LINE, LINE, 6, 10.0)                 # a cap: 6 terms, the two missing ones count as 10
    assert mean.tolist() == [31.0 / 6.0, 29.0 / 6.0, 29.0 / 6.0, 37.0 / 6.0] and kth.tolist() == [10.0] * 4


def test_radius_count_includes_itself_and_the_boundary():
    assert R.radius_count(LINE, LINE, 2.0, 99).tolist() == [2, 3, 2, 1]        # |1 - 3| = 2 counts: <=
    assert R.radius_count(LINE, LINE, 1.999, 99).tolist() == [2, 2, 1, 1]
    assert R.radius_count(LINE, LINE, 100.0, 3).tolist() == [3, 3, 3, 3]


def test_identical_points_are_all_kept():
    p = np.full((5, 3), 0.25, np.float32)
    keep, info = R.remove_outliers(p, nb_neighbors=2, std_ratio=0.0)
    assert keep.all() and info["mu"] == 0.0 and info["sigma"] == 0.0 and info["threshold"] == 0.0
    keep, _ = R.remove_outliers(p[:1], nb_neighbors=3)
    assert keep.tolist() == [True]
    assert R.remove_outliers(p[:0], nb_neighbors=3)[0].shape == (0,)


def test_both_filters_judge_the_input_cloud():
    # a tight cluster, a pair next to it, a far point
    rs = np.random.RandomState(0)
    p = np.concatenate([rs.uniform(0, 0.1, (40, 3)), [[0.5, 0, 0], [0.52, 0, 0]], [[3, 3, 3]]]).astype(np.float32)
    stat, _ = R.remove_outliers(p, nb_neighbors=4, std_ratio=1.0)
    rad, _ = R.remove_outliers(p, radius=0.2, min_neighbors=2)
    both, info = R.remove_outliers(p, nb_neighbors=4, std_ratio=1.0, radius=0.2, min_neighbors=2)
    assert np.array_equal(both, stat & rad)
    assert not stat[-1] and not rad[-1] and not rad[40] and not rad[41] and stat[:40].all() and rad[:40].all()
    assert info["removed_statistical"] == int((~stat).sum()) and info["removed_radius"] == 3


def _sum_by_scalar_loops(x):
    """The order of include/cds_mvsnet_hip.h with Python floats, one addition at a time."""
    x = [float(v) for v in x]
    total = 0.0
    for c in range((len(x) + 4095) // 4096):
        lane = [0.0] * 256
        for l in range(256):
            for r in range(16):
                i = c * 4096 + r * 256 + l
                lane[l] += x[i] if i < len(x) else 0.0
        s = 128
        while s >= 1:
            for l in range(s):
                lane[l] += lane[l + s]
            s //= 2
        total += lane[0]
    return total


def test_fixed_order_sum_is_the_stated_order():
    rs = np.random.RandomState(1)
    x = rs.randn(9000) * 10.0 ** rs.uniform(-8, 8, 9000)
    got = R.fixed_sum(x)
    assert got == _sum_by_scalar_loops(x)
    seq = 0.0
    for v in x:
        seq += float(v)
    assert got != seq and got != float(np.sum(x))         # the array is one where the order shows
    # a case small enough to follow: lane 0 adds 1e16 then 1 (lost), lane 1 holds -1e16; in sequence the 1 survives
    y = np.zeros(300)
    y[0], y[1], y[256] = 1e16, -1e16, 1.0
    assert R.fixed_sum(y) == 0.0 and (1e16 + -1e16) + 1.0 == 1.0
    for n in (1, 2, 255, 4095, 4096, 4097):
        assert R.fixed_sum(x[:n]) == _sum_by_scalar_loops(x[:n])
    mu, sigma = R.stats(np.array([1.0, 2.0, 3.0, 4.0]))
    assert mu == 2.5 and sigma == np.sqrt(5.0 / 3.0)
    assert R.stats(np.array([7.0])) == (7.0, 0.0)


def test_symbols_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "cds_mvsnet_hip.h")).read()
    makefile = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "Makefile")).read()
    for name, nargs in (("cds_knn_mean_f64", 16), ("cds_radius_count_f32", 15), ("cds_outlier_stats_f64", 6),
                        ("cds_knn_mean_wg_f64", 17)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\);", header, re.M | re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.load(), name)
    assert int(re.search(r"#define CDS_KNN_MAX_K (\d+)", header).group(1)) == pointcloud.KNN_MAX_K == 64
    assert int(re.search(r"#define CDS_STAT_CHUNK (\d+)", header).group(1)) == R.CHUNK
    assert re.search(r"^SRCS\s*=.*\bcloud_outlier\.hip\b", makefile, re.M)
    src = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "cloud_outlier.hip")).read()
    assert '#include "grid_common.hpp"' in src
    assert not re.search(r"\basm\b|__asm", src)
    assert not re.search(r"atomic(Add|CAS|Max|Min|Exch)", src)


def test_argument_errors():
    for kw, word in ((dict(nb_neighbors=64), "nb_neighbors"), (dict(nb_neighbors=-1), "nb_neighbors"),
                     (dict(nb_neighbors=5, std_ratio=-0.1), "std_ratio"), (dict(nb_neighbors=5, std_ratio=float("nan")), "std_ratio"),
                     (dict(nb_neighbors=5, std_ratio=float("inf")), "std_ratio"), (dict(radius=-1.0, min_neighbors=2), "radius"),
                     (dict(radius=1.0, min_neighbors=-1), "min_neighbors"), (dict(radius=1.0), "min_neighbors"),
                     (dict(nb_neighbors=5, max_dist=0.0), "max_dist"), (dict(max_dist=2.0), "max_dist"),
                     (dict(radius=0.5, min_neighbors=2, max_dist=2.0), "max_dist"), (dict(min_neighbors=3), "min_neighbors"),
                     (dict(nb_neighbors=5, min_neighbors=3), "min_neighbors")):
        with pytest.raises(ValueError, match=word):
            pointcloud.check_outlier_args(**kw)
    pointcloud.check_outlier_args()
    pointcloud.check_outlier_args(nb_neighbors=63, std_ratio=0.0, radius=0.1, min_neighbors=1, max_dist=2.0)


def test_cli_flags(capsys):
    off = dict(outlier_nb=0, outlier_std=2.0, outlier_radius=0.0, outlier_min_nb=0, outlier_max_dist=None)
    on = ["--outlier_nb", "20", "--outlier_std", "1.5", "--outlier_radius", "0.25", "--outlier_min_nb", "6",
          "--outlier_max_dist", "3"]
    want = dict(outlier_nb=20, outlier_std=1.5, outlier_radius=0.25, outlier_min_nb=6, outlier_max_dist=3.0)
    for mod, io in ((fusion, _IO), (infer, _IO + ["--fuse"]), (gipuma, _IO[2:])):
        a = mod.parse_args(io)
        assert fusion.outlier_kwargs(a) == off == a.outliers
        a = mod.parse_args(io + on)
        assert fusion.outlier_kwargs(a) == want == a.outliers
        for bad, word in ((["--outlier_nb", "64"], "--outlier_nb"), (["--outlier_nb", "-1"], "--outlier_nb"),
                          (["--outlier_nb", "8", "--outlier_std", "-1"], "--outlier_std"),
                          (["--outlier_nb", "8", "--outlier_std", "nan"], "--outlier_std"),
                          (["--outlier_radius", "-0.1", "--outlier_min_nb", "2"], "--outlier_radius"),
                          (["--outlier_radius", "0.1"], "--outlier_min_nb"),
                          (["--outlier_radius", "0.1", "--outlier_min_nb", "-2"], "--outlier_min_nb"),
                          (["--outlier_min_nb", "3"], "--outlier_radius"),
                          (["--outlier_nb", "8", "--outlier_max_dist", "0"], "--outlier_max_dist"),
                          (["--outlier_max_dist", "2"], "--outlier_nb")):
            capsys.readouterr()
            with pytest.raises(SystemExit) as e:
                mod.parse_args(io + bad)
            assert e.value.code == 2, bad
            assert word in capsys.readouterr().err, bad
    # the cloud options are what they were
    a = fusion.parse_args(_IO + on)
    assert fusion.cloud_kwargs(a) == dict(normals=False, normal_radius=2, normal_jump=0.01, normal_min_pts=6, merge_voxel=None,
                                          merge_min_points=1)
    # infer cleans the cloud of --fuse; fusion --from_ply needs a filter and no --testpath
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        infer.parse_args(_IO + ["--outlier_nb", "8"])
    assert e.value.code == 2 and "--fuse" in capsys.readouterr().err
    a = fusion.parse_args(_IO[2:] + ["--from_ply", "x/{scan}.ply", "--outlier_nb", "8"])
    assert a.from_ply == "x/{scan}.ply" and a.testpath is None
    for bad, word in ((_IO[2:] + ["--from_ply", "x/{scan}.ply"], "--from_ply"), (_IO[2:], "--testpath")):
        with pytest.raises(SystemExit) as e:
            fusion.parse_args(bad)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_format_outliers():
    assert fusion.format_outliers({}) == "" and fusion.format_outliers({"points": 3, "merged_from": 9}) == ""
    assert fusion.format_outliers({"outliers_removed": 12, "threshold": 0.0321}) == ", outliers removed 12 (threshold 0.0321)"
    assert fusion.format_outliers({"outliers_removed": 12, "threshold": None}) == ", outliers removed 12"
    assert fusion.format_cloud({"outliers_removed": 12, "threshold": 0.5}) == ""
