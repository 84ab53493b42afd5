"""Trajectory alignment of tt_eval without a GPU: the ``.log`` reader and writer, camera poses from ``cams`` folders, the
sampler of the numpy restatement (tests/tt_traj_ref.py), the declarations of the new C entry point, and the command line's
refusals, all of which come before any device call."""
import os
import re

import numpy as np
import pytest

import tt_traj_ref as TR
from cds_mvsnet_amd import _lib, mvs_io, synth, tt_eval
from test_tt_eval_cpu import _tt_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _poses(m, seed):
    rs = np.random.RandomState(seed)
    out = np.tile(np.eye(4), (m, 1, 1))
    for i in range(m):
        q, _ = np.linalg.qr(rs.randn(3, 3))
        out[i, :3, :3] = q * np.sign(np.linalg.det(q))
        out[i, :3, 3] = rs.uniform(-30, 30, 3)
    return out


def test_log_round_trip(tmp_path):
    poses = _poses(7, 1)
    poses[3, 0, 3] = 1.0 / 3.0                                        # not representable in a few digits
    path = tmp_path / "Barn.log"
    tt_eval.write_log_trajectory(str(path), poses)
    lines = path.read_text().splitlines()
    assert len(lines) == 35 and lines[0] == "0 0 0" and lines[30] == "6 6 0"
    got = tt_eval.read_log_trajectory(str(path))
    assert got.dtype == np.float64 and np.array_equal(got, poses)
    # blank lines between cameras and other metadata integers read the same
    path.write_text("\n".join(ln if i % 5 else f"{i} {i + 1} 42\n" for i, ln in enumerate(lines)) + "\n\n")
    assert np.array_equal(tt_eval.read_log_trajectory(str(path)), poses)
    (tmp_path / "empty.log").write_text("")
    assert tt_eval.read_log_trajectory(str(tmp_path / "empty.log")).shape == (0, 4, 4)
    with pytest.raises(ValueError, match="M,4,4"):
        tt_eval.write_log_trajectory(str(path), np.eye(4))


@pytest.mark.parametrize("line,text,what", [(7, "0.5 0.25 oops 1", "four numbers"), (8, "1 0 0", "four numbers"),
                                            (6, "1 1", "three integers"), (6, "1.5 1 0", "three integers"),
                                            (11, None, "matrix rows")])
def test_a_malformed_log_names_its_line(tmp_path, line, text, what):
    path = tmp_path / "bad.log"
    tt_eval.write_log_trajectory(str(path), _poses(3, 2))
    lines = path.read_text().splitlines()
    if text is None:
        lines = lines[:13]                                            # the third camera (metadata on line 11) loses two rows
    else:
        lines[line - 1] = text
    path.write_text("\n".join(lines) + "\n")
    with pytest.raises(ValueError, match=re.escape(f"{path}:{line}:") + ".*" + what):
        tt_eval.read_log_trajectory(str(path))


def _write_cam(path, pose):
    cam = np.zeros((2, 4, 4), np.float32)
    cam[0] = np.linalg.inv(pose).astype(np.float32)
    cam[1, :3, :3] = [[500, 0, 320], [0, 500, 240], [0, 0, 1]]
    cam[1, 3] = [1.0, 0.01, 192, 3.0]
    mvs_io.write_cam_file(str(path), cam)


def test_camera_poses_from_cams(tmp_path):
    cams = tmp_path / "cams"
    cams.mkdir()
    poses = _poses(4, 3)
    for i, ident in enumerate([12, 0, 7, 3]):                          # written out of order: read back in ascending id
        _write_cam(cams / f"{ident:08d}_cam.txt", poses[i])
    (cams / "pair.txt").write_text("0\n")                             # other files are ignored
    (cams / "0000001_cam.txt").write_text("not a camera")              # seven digits: not a camera file of the layout
    got = tt_eval.camera_poses_from_cams(str(cams))
    assert got.shape == (4, 4, 4) and got.dtype == np.float64
    for k, i in enumerate([1, 3, 2, 0]):
        # the file holds float32 of the inverse: centres of size 30 come back to a few float32 ulp of 30 per coordinate
        assert np.abs(got[k] - poses[i]).max() < 30 * 4 * 2.0 ** -23, k
        w2c = mvs_io.read_cam_file(str(cams / f"{[12, 0, 7, 3][i]:08d}_cam.txt"))[1]
        assert np.array_equal(got[k], np.linalg.inv(w2c.astype(np.float64)))
    with pytest.raises(FileNotFoundError, match="no %08d_cam.txt"):
        tt_eval.camera_poses_from_cams(str(tmp_path))
    with pytest.raises(FileNotFoundError):
        tt_eval.camera_poses_from_cams(str(tmp_path / "nowhere"))


def test_splitmix64_and_the_sampler_are_the_stated_arithmetic():
    # the published first outputs of splitmix64 from state 0: counter c is the (c + 1)-th of them
    assert TR.splitmix64(0, 0) == 0xE220A8397B1DCDAF and TR.splitmix64(0, 1) == 0x6E789E6AA1B965F4
    assert TR.splitmix64(2 ** 64 - 1, 2 ** 64 - 1) == TR.splitmix64(2 ** 64 - 1, -1) < 2 ** 64      # everything is mod 2^64
    for k in (3, 6, 8):
        for n in (k, k + 1, 64, 300):
            for h in (0, 1, 255, 256, 99_999, 2 ** 31 - 2):
                s = TR.sample(9, h, n, k)
                assert len(s) == k == len(set(s)) and min(s) >= 0 and max(s) < n, (k, n, h, s)
                assert s == TR.sample(9, h, n, k)
    assert TR.sample(9, 4, 300, 6) != TR.sample(10, 4, 300, 6) and TR.sample(9, 4, 300, 6) != TR.sample(9, 5, 300, 6)
    assert sorted(TR.sample(3, 5, 6, 6)) == list(range(6))
    # hand-worked: n = 5, picks so far {1, 3}; r = 1 -> skips 1 -> 2; r = 2 -> skips 1 (2 -> 3), then 3 (-> 4)
    for r, want in ((0, 0), (1, 2), (2, 4)):
        got = r
        for p in (1, 3):
            if p <= got:
                got += 1
        assert got == want


@pytest.mark.parametrize("n,k", [(7, 6), (64, 3), (300, 6), (150, 8)])
def test_the_sampler_hits_every_index_at_the_expected_rate(n, k):
    """H samples of k of n without replacement: index i is in a sample with probability p = k / n, and two indices are
    in it together with probability p (k - 1) / (n - 1), so the counts O_i (samples that hold i) have covariance
    H p (1 - p) n / (n - 1) (I - 11^T / n).  With E = H p, X = sum (O_i - E)^2 / E is therefore (1 - p) n / (n - 1) times a
    chi-square variable with n - 1 degrees of freedom (asymptotically in H): X (n - 1) / (n - k) is compared with that
    distribution's mean plus six standard deviations, (n - 1) + 6 sqrt(2 (n - 1)).  A fair sampler exceeds it about once in
    10^8 seeds; one that favours an index by a tenth fails at this H.  Each position of the draw order is uniform over n on
    its own: the plain chi-square statistic with the same bound."""
    H = 20_000
    s = TR.samples(17, H, n, k)
    assert s.shape == (H, k) and s.min() == 0 and s.max() == n - 1
    assert (np.sort(s, 1)[:, 1:] != np.sort(s, 1)[:, :-1]).all()
    obs = np.bincount(s.reshape(-1), minlength=n)
    E = H * k / n
    X = ((obs - E) ** 2 / E).sum() * (n - 1) / (n - k)
    bound = (n - 1) + 6.0 * np.sqrt(2.0 * (n - 1))
    assert X < bound, (X, bound)
    # every position of the draw order is uniform as well (an insertion bug shows in the later draws first)
    for j in (0, k - 1):
        oj = np.bincount(s[:, j], minlength=n)
        Xj = ((oj - H / n) ** 2 / (H / n)).sum()
        assert Xj < bound, (j, Xj, bound)


def test_reference_ransac_recovers_a_similarity_and_orders_the_winner():
    src, dst, S, inl = TR.similarity_data(64, 0.2, 5)
    r = TR.ransac(src, dst, 0.2, 6, 300, 0)
    assert r["count"].max() == inl.sum() == r["count"][r["index"]]
    assert np.abs(r["transform"] - S).max() < 2e-3                      # six noisy pairs, no refit
    tied = np.nonzero(r["count"] == r["count"].max())[0]
    assert r["err2"][r["index"]] == r["err2"][tied].min()
    assert TR.better(3, 1.0, 9, 2, 0.0, 0) and TR.better(3, 0.5, 9, 3, 1.0, 0) and TR.better(3, 1.0, 4, 3, 1.0, 9)
    assert not TR.better(3, 1.0, 9, 3, 1.0, 4) and TR.better(0, 0.0, 7, 0, np.inf, 0)
    # n = k: every hypothesis is the same set, in another order
    few = TR.ransac(src[:6], dst[:6], 0.2, 6, 50, 1)
    assert (np.sort(TR.samples(1, 50, 6, 6), 1) == np.arange(6)).all() and few["ratio"].std() < 1e-9
    # collinear: everything rejected
    line = np.outer(np.linspace(0, 1, 20), [1.0, 2.0, -1.0])
    r = TR.ransac(line, 2 * line + 1, 0.2, 6, 100, 0)
    assert r["index"] == -1 and (r["count"] == 0).all() and np.isinf(r["err2"]).all() and np.array_equal(r["transform"], np.eye(4))
    assert TR.ransac(src[:5], dst[:5], 0.2, 6, 10, 0)["index"] == -1 and TR.ransac(src, dst, 0.2, 6, 0, 0)["index"] == -1


def test_the_new_symbol_is_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "cds_mvsnet_hip.h")).read()
    makefile = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "Makefile")).read()
    m = re.search(r"^int\s+cds_ransac_similarity_f64\s*\(([^;]*?)\);", header, re.M | re.S)
    assert m and len(m.group(1).split(",")) == 13 == len(_lib.SIGNATURES["cds_ransac_similarity_f64"])
    assert hasattr(_lib.load(), "cds_ransac_similarity_f64")
    assert re.search(r"^SRCS\s*=.*\bransac\.hip\b", makefile, re.M)              # built with the library's flags
    assert re.search(r"^%\.o:.*\bransac_common\.hpp\b", makefile, re.M)
    assert int(re.search(r"#define CDS_RANSAC_RECORD (\d+)", header).group(1)) == _lib.RANSAC_RECORD
    assert int(re.search(r"#define CDS_RANSAC_MIN_SAMPLE (\d+)", header).group(1)) == _lib.RANSAC_MIN_SAMPLE == 3
    assert int(re.search(r"#define CDS_RANSAC_MAX_SAMPLE (\d+)", header).group(1)) == _lib.RANSAC_MAX_SAMPLE == 8
    src = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "ransac_common.hpp")).read()
    assert "COLLINEAR_RATIO = 1e-9" in src and TR.COLLINEAR_RATIO == 1e-9


def _args(tmp_path, *extra):
    return ["--datapath", str(tmp_path / "data"), "--plydir", str(tmp_path / "out"), "--scenes", "Barn", *extra]


def test_cli_flag_conflicts(tmp_path, capsys):
    for extra in (("--traj", "a.log", "--cams", "c"), ("--traj", "a.log", "--init", "i.txt"), ("--cams", "c", "--init", "i.txt"),
                  ("--export-log", str(tmp_path / "logs")), ("--export-log", str(tmp_path / "logs"), "--traj", "a.log")):
        with pytest.raises(SystemExit) as e:
            tt_eval.main(_args(tmp_path, *extra))
        assert e.value.code == 2, extra
        err = capsys.readouterr().err
        assert "not allowed with" in err or "--export-log needs --cams" in err, extra
    assert not (tmp_path / "logs").exists()


def test_cli_resolves_the_sfm_log_and_the_trajectory_before_any_device_call(tmp_path, monkeypatch):
    from cds_mvsnet_amd import fusion
    sc = synth.make_tt_scene(n_gt=400, n_pred=300, seed=1)
    _tt_layout(tmp_path / "data", "Barn", sc)
    (tmp_path / "out").mkdir()
    fusion.write_ply(str(tmp_path / "out" / "Barn.ply"), sc["pred"], np.zeros_like(sc["pred"], np.uint8))
    cams = tmp_path / "scan" / "Barn" / "cams"
    cams.mkdir(parents=True)
    _write_cam(cams / "00000000_cam.txt", np.eye(4))

    def no_device(*a, **k):
        raise AssertionError("a device call before the files were resolved")
    monkeypatch.setattr(tt_eval.torch.cuda, "device", no_device)
    monkeypatch.setattr(tt_eval, "ransac_similarity", no_device)
    sfm = str(tmp_path / "data" / "Barn" / "Barn_COLMAP_SfM.log")
    for extra in (("--cams", str(tmp_path / "scan" / "{scene}" / "cams")), ("--traj", str(tmp_path / "{scene}.log"))):
        with pytest.raises(FileNotFoundError, match=re.escape(sfm)):
            tt_eval.main(_args(tmp_path, *extra))
    tt_eval.write_log_trajectory(sfm, _poses(3, 4))
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path / "Barn.log"))):
        tt_eval.main(_args(tmp_path, "--traj", str(tmp_path / "{scene}.log")))
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path / "scan" / "Truck" / "cams"))):
        tt_eval.main(_args(tmp_path, "--cams", str(tmp_path / "scan" / "Truck" / "cams")))


def test_a_camera_count_mismatch_raises_with_both_counts(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the counts are compared before anything is uploaded")
    monkeypatch.setattr(tt_eval, "ransac_similarity", no_device)
    with pytest.raises(ValueError, match="31 estimated cameras against 30 reference cameras"):
        tt_eval.trajectory_alignment(_poses(31, 5), _poses(30, 6), np.eye(4))
    with pytest.raises(ValueError, match="M,4,4"):
        tt_eval.trajectory_alignment(np.eye(4), _poses(30, 6), np.eye(4))


def test_host_tensors_and_bad_arguments_are_refused():
    import torch
    z = torch.zeros(8, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt_eval.ransac_similarity(z, z, 0.2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt_eval.trajectory_alignment(_poses(8, 1), _poses(8, 2), np.eye(4), device="cpu")
