"""Trajectory alignment on the MI355X: cds_ransac_similarity_f64 against the numpy restatement (tests/tt_traj_ref.py) per
hypothesis and for the winner, on geometry that breaks SVD code, for reproducibility, and through the command line from a
moved reconstruction to its F-score.

The restatement and the kernel share every operation before the SVD and after it; np.linalg.svd and the in-lane Jacobi
iteration legitimately differ on a near-collinear sample, so hypotheses whose reference singular-value ratio d2 / d1 is
<= 1e-6 are left out of the per-hypothesis comparison (never more than 1 % of a case: asserted from the reference alone)."""
import functools
import json

import numpy as np
import pytest
import torch

import tt_traj_ref as TR
from cds_mvsnet_amd import fusion, mvs_io, synth, tt_eval
from test_tt_eval_cpu import _tt_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR = 0.2                      # the toolbox's threshold; the clouds span a few units
HS = (1, 63, 64, 65, 256, 257, 1000)
EPS = 2.0 ** -52


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


def _run(src, dst, thr, k, H, seed):
    T, info, count, err2 = tt_eval.ransac_similarity(_d(src), _d(dst), thr, k, H, seed, return_all=True)
    assert count.dtype == torch.int32 and err2.dtype == torch.float64 and count.shape == err2.shape == (H,)
    return T, info, count.cpu().numpy(), err2.cpu().numpy()


def _rel(got, want):
    """|got - want| / |want| elementwise; equal values (0 and 0, inf and inf) give 0."""
    with np.errstate(all="ignore"):
        return np.where(got == want, 0.0, np.abs(got - want) / np.abs(want))


def _ref_winner(ref, H):
    order = np.lexsort((np.arange(H), ref["err2"][:H], -ref["count"][:H].astype(np.int64)))
    return int(order[0])


def _check(src, dst, thr, k, H, seed, ref, err2_tol=None):
    """One launch against the first H rows of the reference table (hypothesis h depends on (seed, h) only).  ``err2_tol``:
    absolute tolerance per hypothesis (default: 1e-9 relative)."""
    T, info, count, err2 = _run(src, dst, thr, k, H, seed)
    keep = ref["ratio"][:H] > 1e-6
    assert 1.0 - keep.mean() <= 0.01
    rc, re = ref["count"][:H], ref["err2"][:H]
    assert np.array_equal(count[keep], rc[keep]), (int((count[keep] != rc[keep]).sum()), H)
    if err2_tol is None:
        rel = _rel(err2[keep], re[keep])
        assert (rel <= 1e-9).all(), (rel.max(), H)
    else:
        fin = keep & ~np.isinf(re)
        assert np.array_equal(np.isinf(err2[keep]), np.isinf(re[keep]))
        assert (np.abs(err2[fin] - re[fin]) <= err2_tol[:H][fin]).all(), float((np.abs(err2[fin] - re[fin]) / err2_tol[:H][fin]).max())
    # the winner by quality, not by index: exact ties (n = k) stay meaningful
    w = _ref_winner(ref, H)
    if np.isinf(re[w]):
        assert info == {"index": -1, "count": 0, "fitness": 0.0, "rmse": 0.0} and np.array_equal(T, np.eye(4))
        return T, info, count, err2
    h = info["index"]
    assert 0 <= h < H and info["count"] == rc[w] == count[h]
    got_e = info["rmse"] ** 2 * info["count"] if info["count"] else 0.0
    tol = 1e-9 * re[w] if err2_tol is None else err2_tol[w]
    assert abs(err2[h] - re[w]) <= tol and abs(got_e - err2[h]) <= 4 * EPS * err2[h]
    assert info["fitness"] == info["count"] / len(src)
    assert np.abs(T - ref["T"][h]).max() <= 1e-9 * np.abs(ref["T"][h]).max() and np.array_equal(T[3], [0, 0, 0, 1])
    return T, info, count, err2


# ------------------------------------------------------------------------------------------------- per-hypothesis parity
@functools.lru_cache(None)
def _parity_case(n, k):
    seed = 1000 * k + n
    src, dst, S, inl = TR.similarity_data(n, THR, seed)
    return src, dst, inl, seed, TR.ransac(src, dst, THR, k, max(HS), seed)


@pytest.mark.parametrize("k", [3, 6, 8])
@pytest.mark.parametrize("n", [6, 7, 64, 300])
def test_every_hypothesis_and_the_winner_match_the_reference(n, k):
    """H at wave and workgroup edges; n = k (every hypothesis the same set, in another order: exact ties up to rounding) and
    n < k (everything rejected).  Data: a random similarity, noise 1e-3 threshold, 40 % of the targets moved by >= 10
    thresholds."""
    src, dst, inl, seed, ref = _parity_case(n, k)
    for H in HS:
        if n < k:
            T, info, count, err2 = _run(src, dst, THR, k, H, seed)
            assert info["index"] == -1 and np.array_equal(T, np.eye(4)) and (count == 0).all() and np.isinf(err2).all()
        else:
            T, info, count, err2 = _check(src, dst, THR, k, H, seed, ref)
    if n >= 64:
        assert info["count"] == inl.sum()                               # 1000 hypotheses find the 60 % at these k


# ---------------------------------------------------------------------------------------------------------- recovery
@functools.lru_cache(None)
def _recovery_case():
    src, dst, S, inl = TR.similarity_data(300, THR, 77)
    return src, dst, S, inl, TR.ransac(src, dst, THR, 6, 100_000, 3)


def test_100000_hypotheses_recover_the_true_inliers():
    src, dst, S, inl, ref = _recovery_case()
    w = ref["index"]
    moved = src[inl] @ ref["transform"][:3, :3].T + ref["transform"][:3, 3]
    assert ref["count"][w] == inl.sum() and np.linalg.norm(moved - dst[inl], axis=1).max() < THR / 10     # the reference does
    T, info = tt_eval.ransac_similarity(_d(src), _d(dst), THR, 6, 100_000, 3)
    assert info["count"] == inl.sum() == 180
    moved = src[inl] @ T[:3, :3].T + T[:3, 3]
    assert np.linalg.norm(moved - dst[inl], axis=1).max() < THR / 10
    assert abs(info["rmse"] ** 2 * info["count"] - ref["err2"][w]) <= 1e-9 * ref["err2"][w]
    assert np.abs(T - ref["T"][info["index"]]).max() <= 1e-9 * np.abs(ref["T"][info["index"]]).max()


# ------------------------------------------------------------------------------------------ geometry that breaks SVD code
def _circle(n, seed, radius=1.0):
    """Cameras on a circle around the object, all in one plane: the covariance of every sample has rank 2."""
    rs = np.random.RandomState(seed)
    a = np.sort(rs.uniform(0, 2 * np.pi, n))
    return np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(n)], 1)


def _moved(src, thr, seed, mirror=False, outlier_frac=0.4):
    rs = np.random.RandomState(seed)
    _, _, S, _ = TR.similarity_data(4, thr, seed)
    dst = src @ S[:3, :3].T + S[:3, 3] + rs.randn(len(src), 3) * (1e-3 * thr)
    out = np.zeros(len(src), bool)
    out[rs.choice(len(src), int(round(outlier_frac * len(src))), replace=False)] = True
    u = rs.randn(len(src), 3)
    dst[out] += (u / np.linalg.norm(u, axis=1, keepdims=True) * rs.uniform(10, 30, (len(src), 1)) * thr)[out]
    if mirror:
        dst = dst * np.array([1.0, 1.0, -1.0])
    return dst, S, ~out


def _conditioned_tol(ref, dst):
    """Absolute tolerance on err2 per hypothesis for the cases below, whose samples are ill-conditioned on purpose.  Both
    sides compute the same covariance from the same sums, so only the SVDs differ: they agree to a few ulp of the
    covariance divided by the sample's conditioning d2 / d1, and T src - dst is then a difference of coordinates of size
    max |dst|.  Each residual component may move by delta = 64 ulp(max |dst|) / ratio, and err2 = sum d_i^2 by at most
    2 delta sqrt(count err2) + count delta^2 (Cauchy-Schwarz).  Counts stay exact."""
    delta = 64 * EPS * np.abs(dst).max() / np.maximum(ref["ratio"], 1e-6)
    c = ref["count"].astype(np.float64)
    return 2 * delta * np.sqrt(c * np.where(np.isinf(ref["err2"]), 0.0, ref["err2"])) + c * delta ** 2


def test_coplanar_cameras_on_a_circle():
    src = _circle(60, 1)
    dst, S, inl = _moved(src, THR, 2)
    ref = TR.ransac(src, dst, THR, 6, 1000, 5)
    for k, r in ((6, ref), (3, TR.ransac(src, dst, THR, 3, 1000, 5))):   # three pairs: rank 2 whatever the cloud
        T, info, _, _ = _check(src, dst, THR, k, 1000, 5, r, err2_tol=_conditioned_tol(r, dst))
        assert info["count"] == inl.sum()
        assert abs(np.linalg.det(T[:3, :3]) - np.linalg.det(S[:3, :3])) < 1e-2 * np.linalg.det(S[:3, :3])   # a rotation, not a mirror


def test_a_mirrored_target_has_no_fit_and_the_counts_still_match():
    src = TR.similarity_data(64, THR, 3)[0]
    dst, S, inl = _moved(src, THR, 4, mirror=True, outlier_frac=0.0)
    ref = TR.ransac(src, dst, THR, 6, 1000, 6)
    T, info, count, _ = _check(src, dst, THR, 6, 1000, 6, ref, err2_tol=_conditioned_tol(ref, dst))
    assert count.max() < len(src) // 2 and np.linalg.det(T[:3, :3]) > 0      # no rotation fits the reflected cloud


def test_an_all_collinear_cloud_rejects_every_hypothesis_and_the_python_layer_raises():
    line = np.outer(np.linspace(-3, 5, 30), [0.6, -0.48, 0.64]) + np.array([1.0, 2.0, 3.0])
    dst = 1.5 * line + 0.25
    T, info, count, err2 = _run(line, dst, THR, 6, 1000, 0)
    assert info == {"index": -1, "count": 0, "fitness": 0.0, "rmse": 0.0} and np.array_equal(T, np.eye(4))
    assert (count == 0).all() and np.isinf(err2).all()
    poses = np.tile(np.eye(4), (30, 1, 1))
    poses[:, :3, 3] = line
    with pytest.raises(ValueError, match="no similarity fits the 30 camera centres"):
        tt_eval.trajectory_alignment(poses, poses, np.eye(4))
    for H, n in ((0, 30), (10, 5)):                                     # no hypothesis; fewer points than a sample
        T, info, count, err2 = _run(line[:n], dst[:n], THR, 6, H, 0)
        assert info["index"] == -1 and info["count"] == 0 and np.array_equal(T, np.eye(4)) and (count == 0).all()
    with pytest.raises(ValueError):
        tt_eval.ransac_similarity(_d(line), _d(dst), THR, k=2)
    with pytest.raises(ValueError):
        tt_eval.ransac_similarity(_d(line), _d(dst[:7]), THR)
    with pytest.raises(ValueError):
        tt_eval.ransac_similarity(_d(line).float(), _d(dst).float(), THR)


def test_centres_at_1e3_with_a_1e_2_threshold():
    """The covariance is a difference of numbers of size 1e6 and the translation one of numbers of size 1e3 times the scale:
    cancellation that both sides share, operation for operation."""
    thr = 1e-2
    src, dst, S, inl = TR.similarity_data(100, thr, 8, offset=1e3)
    ref = TR.ransac(src, dst, thr, 6, 1000, 2)
    T, info, _, _ = _check(src, dst, thr, 6, 1000, 2, ref, err2_tol=_conditioned_tol(ref, dst))
    assert info["count"] == inl.sum()
    moved = src[inl] @ T[:3, :3].T + T[:3, 3]
    assert np.linalg.norm(moved - dst[inl], axis=1).max() < thr / 10


# ------------------------------------------------------------------------------------------------------ reproducibility
def test_two_runs_and_a_side_stream_return_identical_bytes():
    src, dst, inl, seed, _ = _parity_case(300, 6)
    s, d = _d(src), _d(dst)
    a = tt_eval.ransac_similarity(s, d, THR, 6, 5000, 11, return_all=True)
    b = tt_eval.ransac_similarity(s, d, THR, 6, 5000, 11, return_all=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = tt_eval.ransac_similarity(s, d, THR, 6, 5000, 11, return_all=True)
    torch.cuda.current_stream().wait_stream(side)
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and a[1] == other[1]
        assert torch.equal(a[2], other[2]) and torch.equal(a[3], other[3])
    assert a[1]["count"] == inl.sum()
    e = tt_eval.ransac_similarity(s, d, THR, 6, 5000, 12, return_all=True)
    assert e[1]["index"] != a[1]["index"] and not torch.equal(a[2], e[2]) and e[1]["count"] == a[1]["count"]
    # the first hypotheses of a longer run are those of a shorter one: h depends on (seed, h) only
    f = tt_eval.ransac_similarity(s, d, THR, 6, 700, 11, return_all=True)
    assert torch.equal(f[2], a[2][:700]) and torch.equal(f[3], a[3][:700])


# ----------------------------------------------------------------------------------------------------------- end to end
N_CAMS = 40
MOVE = synth.similarity(140.0, (0.5, -0.3, 0.8), (12.0, -7.0, 30.0), 2.6)       # the user's SfM frame: S maps the benchmark's onto it


def moved_scene():
    """A small scene in the T&T layout plus trajectories: the benchmark's reconstruction frame is the prediction frame of
    synth.make_tt_scene (``trans`` maps it onto the scan); 40 cameras stand on a wobbling circle around the object there
    (<Scene>_COLMAP_SfM.log).  The user's reconstruction is the same cloud and the same cameras in another frame, moved by
    the similarity MOVE, its camera centres off by N(0, tau / 4) of the scan's units."""
    sc = synth.make_tt_scene(n_gt=6000, n_pred=5000, tau=0.02, hole_radius=4.0, seed=4)
    rs = np.random.RandomState(9)
    a = np.linspace(0, 2 * np.pi, N_CAMS, endpoint=False)
    centre = np.array([1.5, -0.8, 0.6])
    c_gt = centre + np.stack([1.2 * np.cos(a), 1.2 * np.sin(a), 0.5 + 0.15 * np.sin(3 * a)], 1)
    inv = np.linalg.inv(sc["trans"])
    ref_poses = np.tile(np.eye(4), (N_CAMS, 1, 1))
    for i in range(N_CAMS):
        ref_poses[i, :3, :3] = synth.similarity(float(np.degrees(a[i])), (0.1, 0.2, 1.0), (0, 0, 0))[:3, :3]
    ref_poses[:, :3, 3] = c_gt @ inv[:3, :3].T + inv[:3, 3]
    scale = np.cbrt(np.linalg.det(MOVE[:3, :3]))
    rot = MOVE[:3, :3] / scale
    est_poses = ref_poses.copy()
    est_poses[:, :3, :3] = rot @ ref_poses[:, :3, :3]
    noisy = ref_poses[:, :3, 3] + rs.randn(N_CAMS, 3) * (sc["tau"] / 4)
    est_poses[:, :3, 3] = noisy @ MOVE[:3, :3].T + MOVE[:3, 3]
    pred = (sc["pred"].astype(np.float64) @ MOVE[:3, :3].T + MOVE[:3, 3]).astype(np.float32)
    return sc, ref_poses, est_poses, pred


def polygon_gap(sc, Ta, Tb):
    """The largest distance between where Ta and Tb map the points that Tb maps onto the crop polygon's vertices (taken at
    the middle of the crop's axis range)."""
    v = np.array(sc["crop"]["bounding_polygon"], np.float64)
    v[:, 2] = 0.5 * (sc["crop"]["axis_min"] + sc["crop"]["axis_max"])
    M = np.asarray(Ta) @ np.linalg.inv(np.asarray(Tb))
    return float(np.linalg.norm(v @ M[:3, :3].T + M[:3, 3] - v, axis=1).max())


def test_cli_aligns_a_moved_reconstruction_from_its_cameras(tmp_path):
    """Checked on the CPU for this scene and seed 5: the restatement (tt_traj_ref.ransac on the centres as the cam files
    hold them, then tt_eval_ref.register) started from the trajectory alignment and from trans @ inv(MOVE) ends 8.6e-5
    apart on the polygon's vertices (tau / 2 = 1e-2; the two starts are 1.8e-3 apart), F-score 0.9016 from both."""
    sc, ref_poses, est_poses, pred = moved_scene()
    tau = sc["tau"]
    data, out, cams = tmp_path / "data", tmp_path / "out", tmp_path / "scan" / "Barn" / "cams"
    _tt_layout(data, "Barn", sc)
    tt_eval.write_log_trajectory(str(data / "Barn" / "Barn_COLMAP_SfM.log"), ref_poses)
    out.mkdir()
    cams.mkdir(parents=True)
    fusion.write_ply(str(out / "Barn.ply"), pred, np.zeros_like(pred, np.uint8))
    for i, pose in enumerate(est_poses):
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0] = np.linalg.inv(pose).astype(np.float32)
        cam[1, :3, :3] = [[500, 0, 320], [0, 500, 240], [0, 0, 1]]
        cam[1, 3] = [1.0, 0.01, 192, 3.0]
        mvs_io.write_cam_file(str(cams / f"{i:08d}_cam.txt"), cam)
    base = ["--datapath", str(data), "--plydir", str(out), "--scenes", "Barn", "--tau", str(tau)]

    plain = tt_eval.main(base)
    assert plain["scenes"]["Barn"]["fscore"] < 0.05 and "trajectory" not in plain["scenes"]["Barn"]
    assert plain["settings"] == {"tau": tau, "register": True}

    init = tmp_path / "init.txt"
    np.savetxt(init, np.linalg.inv(MOVE), fmt="%.17g")
    exact = tt_eval.main(base + ["--init", str(init)])["scenes"]["Barn"]
    assert exact["fscore"] > 0.2

    logs = tmp_path / "logs"
    res = tt_eval.main(base + ["--cams", str(tmp_path / "scan" / "{scene}" / "cams"), "--export-log", str(logs), "--seed", "5",
                               "--json", str(tmp_path / "r.json")])
    got = res["scenes"]["Barn"]
    tr = got["trajectory"]
    assert set(tr) == {"index", "count", "fitness", "rmse", "transform"} and res["settings"]["seed"] == 5
    assert tr["count"] == N_CAMS and tr["fitness"] == 1.0 and 0 < tr["rmse"] < tau and 0 <= tr["index"] < 100_000
    start = sc["trans"] @ np.linalg.inv(MOVE)
    assert polygon_gap(sc, tr["transform"], start) < 2 * tau           # six cameras off by tau / 4 each, no refit
    gap = polygon_gap(sc, got["transform"], exact["transform"])
    print(f"\nfinal transforms from --cams and from the exact start: {gap:.3e} apart on the polygon (tau / 2 = {tau / 2:g}); "
          f"f-score {got['fscore']:.4f} vs {exact['fscore']:.4f}")
    assert gap < tau / 2
    assert json.load(open(tmp_path / "r.json"))["scenes"]["Barn"]["trajectory"] == tr

    # the exported log is the reconstruction's trajectory; scoring from it gives the identical result
    assert np.array_equal(tt_eval.read_log_trajectory(str(logs / "Barn.log")), tt_eval.camera_poses_from_cams(str(cams)))
    again = tt_eval.main(base + ["--traj", str(logs / "{scene}.log"), "--seed", "5"])["scenes"]["Barn"]
    assert again["trajectory"] == tr and again["transform"] == got["transform"]
    for k in ("precision", "recall", "fscore", "precision_curve", "recall_curve", "n_pred_sampled", "n_gt_sampled"):
        assert again[k] == got[k], k

    # one camera fewer in the estimate: both counts in the message
    (cams / f"{N_CAMS - 1:08d}_cam.txt").unlink()
    with pytest.raises(ValueError, match=f"{N_CAMS - 1} estimated cameras against {N_CAMS} reference cameras"):
        tt_eval.main(base + ["--cams", str(cams)])
