"""Host side of the depth-map evaluation (cds_mvsnet_amd/depth_eval.py): the float64 restatement the GPU tests compare against
reproduces what the REFERENCE's own metric functions returned (golden set G16), the OpenCV index rule, the crop tables of the two
dataset layouts, the command lines, and the C ABI bookkeeping of the two new entry points.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import depth_eval_ref as R
from conftest import GOLDEN, ROOT

# worst case of ANY float32 summation order against float64 over n <= 4096 terms: n 2^-24
REL = 4096 * 2.0 ** -24


@pytest.fixture(scope="module")
def g16():
    z = np.load(os.path.join(GOLDEN, "g16_depth_metrics.npz"))
    return {k: z[k] for k in z.files}


def close(got, want, rel=REL):
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= rel * abs(want)


def test_restatement_reproduces_the_reference_scalars(g16):
    assert tuple(g16["names"]) == R.NAMES
    for tag in ("a", "b"):
        est, gt, mask, iv = (g16[f"{tag}_{k}"] for k in ("est", "gt", "mask", "interval"))
        assert max(int((m > 0.5).sum()) for m in mask) <= 4096
        got = R.validation_scalars(est, gt, mask, iv[0])
        for k, want in zip(R.NAMES, g16[f"{tag}_validation"]):
            assert close(got[k], float(want)), (tag, k, got[k], float(want))
        gotp = R.precision_scalars(est, gt, mask)
        for k, want in zip(R.PRECISION_NAMES, g16[f"{tag}_precision"]):
            assert close(gotp[k], float(want)), (tag, k, gotp[k], float(want))
    # the empty mask: NaN for the means over the mask, 0 for every band
    assert all(math.isnan(v) for v in g16["b_validation"][:6]) and (g16["b_validation"][6:] == 0).all()


def test_counts_match_the_reference_exactly(g16):
    """The count-only scalars (thres*_error, thresh*mm_error) are ratios of integers < 2^24: float32 holds them exactly up to the final
    division and the batch mean, so the pixel COUNTS of the restatement must equal the reference's.  The fixture has pixels exactly
    on float32(threshold) and one ulp either side: a double-precision comparison, or a band that excludes an end, changes a count."""
    est, gt, mask, iv = (g16[f"a_{k}"] for k in ("est", "gt", "mask", "interval"))
    di = float(iv[0]) / 2.65
    thr = [di * m for m in R.MULTIPLIERS]
    sums = R.metric_sums(est, gt, mask, thr, R.CAP)
    n = sums[:, 0]
    for t in range(5):
        # float32 per-image ratio, float32 mean over the two images: the reference's arithmetic on the restatement's counts
        ratio = (sums[:, 3 + t].astype(np.float32) / n.astype(np.float32)).astype(np.float32)
        want = np.float32(g16["a_validation"][1 + t])
        assert np.float32(ratio.astype(np.float32).mean(dtype=np.float32)) == want, t
    psums = R.metric_sums(est, gt, mask, [1.0, 2.0, 4.0], R.CAP)
    for t in range(3):
        within = [1.0 - float(np.float32(psums[b, 3 + t]) / np.float32(psums[b, 0])) for b in range(2)]      # precision.py:13
        assert np.mean(within) == g16["a_precision"][2 + t], t
    # on-threshold pixels: e == float32(thr) is not "> thr" but lies in both neighbouring bands
    e0 = R._errors(est[0], gt[0], mask[0])
    for t in (1, 3):
        t32 = np.float32(thr[t])
        assert np.count_nonzero(e0 == t32) >= 2 and np.count_nonzero(e0 == np.nextafter(t32, np.float32(np.inf))) >= 2
        assert np.count_nonzero(e0 == np.nextafter(t32, np.float32(0))) >= 2
    counts = sums[:, 3 + 5::2]
    assert (counts[0] > 0).all() and list(np.flatnonzero(counts[1] == 0)) == [2, 4]
    # bands overlap on their shared ends: the band counts add up to n plus the on-threshold pixels
    on = sum(np.count_nonzero(e0 == np.float32(x)) for x in thr)
    assert counts[0].sum() == n[0] + on


def test_host_scalars_from_sums_equal_the_restatement(g16):
    """depth_eval forms its scalars on the host from the kernel's sums: fed the restatement's sums it must return the restatement's
    scalars (same float64 arithmetic), NaN and empty bands included."""
    from cds_mvsnet_amd import depth_eval as E
    assert E.VALIDATION_NAMES == R.NAMES and E.PRECISION_NAMES == R.PRECISION_NAMES
    for tag in ("a", "b"):
        est, gt, mask, iv = (g16[f"{tag}_{k}"] for k in ("est", "gt", "mask", "interval"))
        di = float(iv[0]) / 2.65
        got = E._validation_from_sums(R.metric_sums(est, gt, mask, [di * m for m in R.MULTIPLIERS], R.CAP))
        want = R.validation_scalars(est, gt, mask, iv[0])
        assert list(got) == list(R.NAMES)
        for k in R.NAMES:
            assert close(got[k], want[k], 1e-12), (tag, k)
        gotp = E._precision_from_sums(R.metric_sums(est, gt, mask, [1.0, 2.0, 4.0], R.CAP))
        wantp = R.precision_scalars(est, gt, mask)
        for k in R.PRECISION_NAMES:
            assert close(gotp[k], wantp[k], 1e-12), (tag, k)
    assert E._validation_thresholds(torch.tensor([2.65, 9.0]), 2, None) == [float(np.float32(2.65)) / 2.65 * m for m in R.MULTIPLIERS]


def mvs_io_index(n_dst, n_src):
    """The rows mvs_io.nearest_resize picks: i * (n_src / n_dst)."""
    from cds_mvsnet_amd import mvs_io
    return mvs_io.nearest_resize(np.arange(n_src, dtype=np.int64).reshape(n_src, 1), n_dst, 1)[:, 0]


def test_nearest_index_is_the_opencv_rule():
    from cds_mvsnet_amd import depth_eval as E
    assert np.array_equal(E.nearest_index(800, 1600), 2 * np.arange(800))
    assert np.array_equal(E.nearest_index(7, 7), np.arange(7))
    for n_dst, n_src in ((1152, 1600), (864, 1200), (8, 21), (16, 37), (48, 40), (5, 1)):
        got = E.nearest_index(n_dst, n_src)
        assert got.dtype == np.int64 and np.array_equal(got, R.nearest_index(n_dst, n_src))
        assert got.min() >= 0 and got.max() <= n_src - 1 and (np.diff(got) >= 0).all()
    # where i * (n_src / n_dst) is an integer the inverse of the forward scale falls just short of it: mvs_io.nearest_resize's
    # rule picks the next pixel
    for n_dst, n_src, i, cv, naive in ((864, 1600, 27, 49, 50), (600, 1080, 15, 26, 27), (20, 576, 15, 431, 432)):
        assert i * n_src % n_dst == 0 and i * n_src // n_dst == naive
        assert E.nearest_index(n_dst, n_src)[i] == cv and int(i * (n_src / n_dst)) == naive == mvs_io_index(n_dst, n_src)[i]
    # 1600 -> 1152 (the size precision.py evaluates at): 1 / (1152 / 1600) and 1600 / 1152 are the same double, the rules agree
    assert 1.0 / (1152 / 1600) == 1600 / 1152 and np.array_equal(E.nearest_index(1152, 1600), mvs_io_index(1152, 1600))
    with pytest.raises(ValueError):
        E.nearest_index(0, 5)


def test_crop_tables_follow_the_two_prepare_img_rules():
    from cds_mvsnet_amd import depth_eval as E
    # DTU (dtu_yao.py:79-94): 1200 x 1600 -> 600 x 800 -> rows 44..555, cols 80..719 of the half-size image = every second pixel
    rows, cols = E.gt_tables(1200, 1600, "dtu")
    assert rows.shape == (512,) and cols.shape == (640,)
    assert np.array_equal(rows, 2 * (np.arange(512) + (600 - 512) // 2)) and np.array_equal(cols, 2 * (np.arange(640) + (800 - 640) // 2))
    # odd source sizes: (h - 512) // 2 on the floor-halved size
    rows, cols = E.gt_tables(1201, 1603, "dtu")
    assert np.array_equal(rows, R.dtu_tables(1201, 1603)[0]) and np.array_equal(cols, R.dtu_tables(1201, 1603)[1])
    assert rows[0] == R.nearest_index(600, 1201)[44] and cols[0] == R.nearest_index(801, 1603)[80]
    # BlendedMVS (blended_dataset.py:79-84): crop only; 576 x 768 is the identity
    rows, cols = E.gt_tables(576, 768, "blended")
    assert np.array_equal(rows, np.arange(576)) and np.array_equal(cols, np.arange(768))
    rows, cols = E.gt_tables(1536, 2048, "blended")
    assert rows[0] == (1536 - 576) // 2 == 480 and cols[0] == (2048 - 768) // 2 == 640 and rows[-1] == 480 + 575 and cols[-1] == 640 + 767
    rows, cols = E.gt_tables(41, 49, "blended", crop=(16, 32))
    assert rows[0] == (41 - 16) // 2 and cols[0] == (49 - 32) // 2 and rows.size == 16 and cols.size == 32
    rows, cols = E.gt_tables(40, 48, "dtu", crop=(16, 16))
    assert np.array_equal(rows, R.dtu_tables(40, 48, (16, 16))[0]) and np.array_equal(cols, R.dtu_tables(40, 48, (16, 16))[1])
    with pytest.raises(ValueError):
        E.gt_tables(600, 800, "dtu")                 # 300 x 400 after halving: smaller than the crop
    with pytest.raises(ValueError):
        E.gt_tables(600, 800, "eth3d")


def test_command_lines():
    from cds_mvsnet_amd import depth_eval as E, infer
    a = E.parse_args(["--gtpath", "g", "--outdir", "o", "--testlist", "l.txt"])
    assert a.folders == ["depth_est"] and a.json is None and a.device == "cuda"
    a = E.parse_args(["--gtpath", "g", "--outdir", "o", "--testlist", "l.txt", "--folders", "depth_est, depth_stage1,depth_stage3",
                      "--json", "out.json"])
    assert a.folders == ["depth_est", "depth_stage1", "depth_stage3"] and a.json == "out.json"
    with pytest.raises(SystemExit):
        E.parse_args(["--gtpath", "g", "--outdir", "o"])
    with pytest.raises(SystemExit):
        E.parse_args(["--gtpath", "g", "--outdir", "o", "--testlist", "l", "--folders", ","])
    b = infer.parse_args(["--testpath", "t", "--testlist", "l", "--outdir", "o"])
    assert b.save_stages is False
    assert infer.parse_args(["--testpath", "t", "--testlist", "l", "--outdir", "o", "--save_stages"]).save_stages is True


def test_cli_names_a_missing_ground_truth_file(tmp_path):
    from cds_mvsnet_amd import depth_eval as E, mvs_io
    os.makedirs(tmp_path / "out" / "scan1" / "depth_est")
    os.makedirs(tmp_path / "gt" / "scan1")
    mvs_io.write_pfm(str(tmp_path / "out" / "scan1" / "depth_est" / "00000003.pfm"), np.ones((4, 6), np.float32))
    with pytest.raises(FileNotFoundError, match="depth_map_0003.pfm"):
        E._folder_jobs(str(tmp_path / "gt"), str(tmp_path / "out"), ["scan1"], "depth_est")
    mvs_io.write_pfm(str(tmp_path / "gt" / "scan1" / "depth_map_0003.pfm"), np.ones((8, 12), np.float32))
    with pytest.raises(FileNotFoundError, match="depth_visual_0003.png"):
        E._folder_jobs(str(tmp_path / "gt"), str(tmp_path / "out"), ["scan1"], "depth_est")
    with pytest.raises(FileNotFoundError, match="depth_stage2"):
        E._folder_jobs(str(tmp_path / "gt"), str(tmp_path / "out"), ["scan1"], "depth_stage2")


def test_no_cpu_path():
    from cds_mvsnet_amd import depth_eval as E, ops
    x = torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError):
        ops.depth_metric_sums(x, x, x, [1.0], 1e5)
    with pytest.raises(RuntimeError):
        ops.gt_pyramid(torch.zeros(4, 4), [0, 1], [0, 1], levels=1)
    with pytest.raises(RuntimeError):
        E.depth_metrics(x, x, x, [1.0])
    with pytest.raises(RuntimeError):
        E.precision_scalars(x, x, x)
    with pytest.raises(RuntimeError):
        E.read_gt_ms("a.pfm", None, "blended", "cpu")


def test_new_symbols_are_declared_everywhere():
    from cds_mvsnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "cds_mvsnet_hip.h")).read()
    makefile = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "Makefile")).read()
    for name, nargs in (("cds_depth_metrics_f32", 12), ("cds_gt_pyramid_f32", 13)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\);", header, re.M | re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert re.search(r"^SRCS\s*=.*\bdepth_metrics\.hip\b", makefile, re.M)
    assert os.path.exists(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "depth_metrics.hip"))
    assert int(re.search(r"#define CDS_DEPTH_METRICS_MAX_T (\d+)", header).group(1)) == _lib.DEPTH_METRICS_MAX_T
    assert int(re.search(r"#define CDS_DEPTH_METRICS_MAX_GROUPS (\d+)", header).group(1)) == _lib.DEPTH_METRICS_MAX_GROUPS
