"""COLMAP -> MVSNet conversion on the MI355X: the two float64 kernels against the restatement (tests/colmap_ref.py),
degenerate geometry, reproducibility, a Tanks-and-Temples-sized score matrix, and the CLI end to end against the files the
REFERENCE wrote for the G15 model, read back by EvalScenes and run through infer.

Bounds.  q = ops.COLMAP_SCORE_QUANTUM = 2^-80 bounds the error with which a term enters the fixed-point score matrix.
With n_ij the number of terms of a pair (occurrences in the lower image counted), every pair must satisfy
|S_gpu - S_ref| <= n_ij (q + 1e-11): the cosine is good to a few ulp, which at theta >= 0.1 degrees (asserted by the generator) is an angle error below ~4e-12
degrees, times max |dw/dtheta| = 0.61 / sigma1, ~1e-12 per term; 1e-11 leaves an order of margin.  With identical poses
theta is ~0, where the angle error grows to sqrt(2 x few ulp) rad ~ 2e-6 degrees while |dw/dtheta| is 5 e^-12.5 ~ 2e-5:
n_ij (q + 1e-10).  depth_min and depth_max: 1e-12 relative."""
import os

import numpy as np
import pytest
import torch

import colmap_ref as R
from cds_mvsnet_amd import colmap, infer, mvs_io, ops, synth
from test_colmap_cpu import RUNS, fixture, fixture_model, scene_files, write_dense

pytestmark = pytest.mark.gpu
Q = ops.COLMAP_SCORE_QUANTUM


def _gpu(model, **kw):
    return colmap.pair_scores(*model, **kw), torch.from_numpy(colmap.depth_ranges(*model))


def _assert_selection(S_gpu, s, bound):
    """The selected ids are those of the restatement.  Equal scores follow one rule on both sides (higher index first), so
    there the ids must be identical.  A deliberate reading of "equal under the tie rule" for float64: two ids may trade
    places (or the last place) only where their RESTATED scores differ by no more than the two pairs' error bounds
    n (q + per_term), i.e. where the order is not decided within the error the score test itself allows; any larger gap
    must be reproduced.  This is far tighter than the %f ties of the comparison with the reference's files."""
    got, want = colmap.select_views(S_gpu), s["view_sel"]
    for i, (g, w) in enumerate(zip(got, want)):
        for (kg, _), (kw, _) in zip(g, w):
            if kg != kw:
                assert abs(s["score"][i, kg] - s["score"][i, kw]) <= bound[i, kg] + bound[i, kw], (i, g, w)


def _check(model, per_term=1e-11, **kw):
    s = R.scene(*model, **kw)
    S, mm = _gpu(model, **{k: v for k, v in kw.items() if k in ("theta0", "sigma1", "sigma2")})
    S = S.cpu().numpy()
    assert np.isfinite(S).all() and np.isfinite(mm.numpy()).all()
    assert np.array_equal(S, S.T) and not S.diagonal().any() and S.max() > 1.0
    bound = s["n_terms"] * (Q + per_term)
    err = np.abs(S - s["score"])
    print(f"pairs {int((s['n_terms'] > 0).sum() // 2)}, terms {s['n_terms'].sum() / 2:.0f}, max |dS| {err.max():.3e}, "
          f"max |dS| / n {np.max(err / np.maximum(s['n_terms'], 1)):.3e}, q {Q:.3e}")
    assert (err <= bound).all(), (err.max(), np.max(err / np.maximum(s["n_terms"], 1)))
    assert np.array_equal(S > 0, s["score"] > 0)         # however small: a pair that shares a point outranks one that shares none
    rel = np.abs(mm.numpy() - s["min_max"]) / np.abs(s["min_max"])
    print(f"depth range max rel err {rel.max():.3e}")
    assert rel.max() <= 1e-12
    _assert_selection(S, s, bound)
    return s, S


def test_quantum_is_the_librarys():
    from cds_mvsnet_amd import _lib
    assert Q == 2.0 ** -_lib.load().cds_colmap_score_quantum_log2() and Q <= 2.0 ** -40
    # limbs: floor(bits / 40) + 2 with w >= 2^-bits over theta in [0, 180]
    assert ops.colmap_score_limbs(5, 1, 10) == 7 and ops.colmap_score_limbs(5, 1, 5) == int(175 ** 2 / 50 * 1.4426950408889634 / 40) + 2
    assert ops.colmap_score_limbs(5, 0.01, 10) == ops.COLMAP_SCORE_MAX_LIMBS == 28 and ops.colmap_score_limbs(5, 1000, 1000) == 2


# --------------------------------------------------------------------------------------------- 4. kernels vs restatement
@pytest.mark.parametrize("ext", [".txt", ".bin"])
def test_fixture_model(tmp_path, ext):
    model, _ = fixture_model(tmp_path, ext)
    _check(model)


# sigma2 = 3: weights down to ~e^-500 = 2^-720, far below the 7 limbs of the defaults: the limbs follow the parameters
@pytest.mark.parametrize("kw", [{}, {"theta0": 8.0, "sigma1": 2.5, "sigma2": 4.0}, {"sigma2": 3.0}])
def test_synthetic_64_images(kw):
    model = synth.make_colmap_model(64, 20_000, seed=1, dup_frac=0.01)          # asserts every theta >= 0.1 degrees
    s, _ = _check(model, **kw)
    assert s["n_terms"].sum() / 2 > 400_000 and np.diff(model[2].track_ptr).max() == 62


def test_indices_out_of_range_raise():
    d = "cuda"
    xyz, ctr = torch.zeros(2, 3, dtype=torch.float64, device=d), torch.ones(3, 3, dtype=torch.float64, device=d)
    with pytest.raises(ValueError, match="outside"):
        ops.colmap_pair_scores(torch.tensor([0, 3], dtype=torch.int32, device=d), torch.tensor([0, 1], device=d), xyz, ctr, 5, 1, 10)
    with pytest.raises(ValueError, match="outside"):
        ops.colmap_pair_scores(torch.tensor([0, 1], dtype=torch.int32, device=d), torch.tensor([0, 2], device=d), xyz, ctr, 5, 1, 10)


# ------------------------------------------------------------------------------------------------ 5. degenerate geometry
def test_identical_poses_and_point_on_a_centre():
    cameras, images, points = synth.make_colmap_model(16, 3000, seed=5, dup_frac=0.01, n_isolated=1, min_angle_deg=None)
    ids = sorted(images)
    a, b, c = ids[4], ids[5], ids[9]
    images[b] = images[b]._replace(qvec=images[a].qvec.copy(), tvec=images[a].tvec.copy())       # two identical poses
    # camera c: identity rotation, so its centre -R^T t = (0.25, -0.5, 1.5) exactly, whoever computes it; a point of its
    # track sits on it
    images[c] = images[c]._replace(qvec=np.array([1.0, 0.0, 0.0, 0.0]), tvec=np.array([-0.25, 0.5, -1.5]))
    pid = images[c].point3D_ids
    k = int(np.searchsorted(points.ids, pid[pid != -1][0]))
    assert np.diff(points.track_ptr)[k] >= 2
    points.xyz[k] = [0.25, -0.5, 1.5]
    shared = np.intersect1d(images[a].point3D_ids, images[b].point3D_ids)
    assert (shared != -1).sum() > 50
    s, S = _check((cameras, images, points), per_term=1e-10)
    assert np.array_equal(s["centres"][9], [0.25, -0.5, 1.5]) and np.array_equal(colmap.scene_cameras(cameras, images)[2][9], [0.25, -0.5, 1.5])
    # theta = 0 between the twins: every shared term is w(0) = exp(-12.5)
    n = s["n_terms"][4, 5]
    assert abs(S[4, 5] - n * np.exp(-12.5)) <= n * (Q + 1e-10) and n > 50


# -------------------------------------------------------------------------------------------------- 6. reproducibility
def test_two_runs_are_bit_identical():
    model = synth.make_colmap_model(64, 20_000, seed=2, dup_frac=0.01)
    (S1, r1), (S2, r2) = _gpu(model), _gpu(model)
    assert torch.equal(S1, S2) and torch.equal(r1, r2) and S1.abs().sum() > 0


def test_300_images_200k_points():
    """Tens of millions of terms, track lengths from 2 to every arc camera."""
    model = synth.make_colmap_model(300, 200_000, seed=2)
    L = np.diff(model[2].track_ptr)
    assert L.max() == 298 and L[L > 0].min() <= 2 and 5.0 < L.mean() < 7.0
    s, _ = _check(model)
    assert s["n_terms"].sum() / 2 > 2e7


# -------------------------------------------------------------------------------------------------------- 7. end to end
def _convert(tmp_path, ext, max_d):
    fx = fixture()
    dense = write_dense(str(tmp_path / "dense"), fx)
    save = str(tmp_path / "scenes" / "scanC")
    out = colmap.main(["--dense_folder", dense, "--save_folder", save, "--max_d", str(max_d), "--model_ext", ext])
    assert out["images"] == 12 and out["points"] == 400
    return fx, dense, save


@pytest.mark.parametrize("ext,max_d", RUNS)
def test_cli_reproduces_reference_files(tmp_path, ext, max_d):
    fx, _, save = _convert(tmp_path, ext, max_d)
    got, want = scene_files(save), fx[(ext, max_d)]
    assert sorted(got) == sorted(want)
    R.assert_same_scene_files(got, want)
    for name, data in want.items():
        if name.startswith("images_post/"):
            assert got[name] == data


def test_eval_scenes_reads_the_scene_and_infer_runs(tmp_path):
    fx, dense, save = _convert(tmp_path, ".bin", 192)
    root = os.path.dirname(save)
    cameras, images, _ = colmap.read_model(os.path.join(dense, "sparse"), ".bin")
    ext, intr, _ = colmap.scene_cameras(cameras, images)
    nd, H, W = 48, 64, 96
    data = mvs_io.EvalScenes(root, ["scanC"], nviews=3, ndepths=nd, interval_scale=1.0, max_h=H, max_w=W, dataset="general")
    assert len(data) == 12
    pairs = mvs_io.read_pair_file(os.path.join(save, "pair.txt"))
    for idx in (0, 7, 11):
        smp = data[idx]
        ref, src = pairs[idx]
        views = [ref] + (src + [src[0]] * 2)[:2]
        assert smp["imgs"].shape == (3, 3, H, W)
        for v, vid in enumerate(views):
            k32 = intr[vid].astype(np.float32)
            k32[:2, :] /= 4.0
            k32[0, :] *= W / 48
            k32[1, :] *= H / 32
            m = smp["proj_matrices"]["stage1"][v]
            assert np.array_equal(m[0], ext[vid].astype(np.float32)) and np.array_equal(m[1, :3, :3], k32)
        f = [float(x) for x in open(os.path.join(save, "cams", "%08d_cam.txt" % ref)).read().split("\n")[11].split()]
        dint = (f[0] + int(f[2]) * f[1] - f[0]) / nd
        assert np.array_equal(smp["depth_values"], np.arange(f[0], dint * (nd - 0.5) + f[0], dint, dtype=np.float32))
        assert f[2] == 192.0 and abs(f[0] + 191 * f[1] - f[3]) < 1e-3
    with open(tmp_path / "list.txt", "w") as fh:
        fh.write("scanC\n")
    out = str(tmp_path / "out")
    infer.main(["--testpath", root, "--testlist", str(tmp_path / "list.txt"), "--outdir", out, "--num_view", "3",
                "--max_h", str(H), "--max_w", str(W), "--interval_scale", "1.0", "--dataset", "general"])
    for i in range(12):
        d = mvs_io.read_pfm(os.path.join(out, "scanC", "depth_est", "%08d.pfm" % i))[0]
        assert d.shape == (H, W) and np.isfinite(d).all() and d.std() > 0
