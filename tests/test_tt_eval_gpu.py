"""Tanks and Temples evaluation on the MI355X: the registration kernels (nearest index, pair sums, voxel mean, polygon crop),
ICP, the three registration rounds and the CLI against the float64 numpy restatement of the rules (tests/tt_eval_ref.py)."""
import functools
import json

import numpy as np
import pytest
import torch

import tt_eval_ref as R
from cds_mvsnet_amd import _lib, fusion, pointcloud, synth, tt_eval
from test_tt_eval_cpu import _tt_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _ulp_close(got, want, ulps=2):
    got = np.asarray(got, np.float32)
    want = np.asarray(want, np.float32)
    tol = ulps * np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))
    return np.abs(got - want) <= tol


# ------------------------------------------------------------------------------------------------------- nearest index
def _index_check(q, t, cap, **kw):
    dist, index = pointcloud.nearest_index(_g(q), _g(t), cap, **kw)
    assert dist.dtype == torch.float32 and index.dtype == torch.int32 and dist.shape == index.shape == (len(q),)
    want_d, want_i = R.nearest_index(q, t, cap)
    got_i = index.cpu().numpy()
    assert np.array_equal(got_i, want_i), (int((got_i != want_i).sum()), got_i[got_i != want_i][:5], want_i[got_i != want_i][:5])
    ok = _ulp_close(dist.cpu().numpy(), want_d)
    assert ok.all(), (int((~ok).sum()), dist.cpu().numpy()[~ok][:5], want_d[~ok][:5])
    return dist.cpu().numpy(), got_i


@pytest.mark.parametrize("m,n", [(1, 1), (1, 5000), (5000, 1), (40_000, 40_000)])
def test_nearest_index_sizes(m, n):
    rs = np.random.RandomState(m % 97 + n % 89)
    t = synth.make_dtu_scene(40, 30, 0.5, 2.0, 2.0)["stl"]
    t = t[rs.choice(len(t), n, replace=n > len(t))] + rs.randn(n, 3).astype(np.float32) * 0.2
    q = t[rs.choice(n, m)] + rs.randn(m, 3).astype(np.float32) * rs.choice([0.1, 1.0, 8.0], (m, 1)).astype(np.float32)
    d, i = _index_check(q.astype(np.float32), t.astype(np.float32), 5.0)
    if m > 1000 and n > 1000:
        assert (i >= 0).any() and (i < 0).any()


def test_nearest_index_duplicates_far_queries_and_empty():
    rs = np.random.RandomState(6)
    base = rs.uniform(-40, 40, (3000, 3)).astype(np.float32)
    t = np.tile(base, (5, 1))                                       # point k again at k + 3000, k + 6000, ...: the first wins
    q = np.concatenate([base[:500], base[500:1500] + rs.randn(1000, 3).astype(np.float32) * 0.5,
                        rs.uniform(-1, 1, (300, 3)).astype(np.float32) * 5e3,            # far outside the grid
                        np.array([[1e6, -1e6, 3e5]], np.float32)])
    d, i = _index_check(q, t, 10.0)
    assert (i[:500] == np.arange(500)).all() and (d[:500] == 0).all()
    assert (i < 3000).all()
    assert (i[1500:] == -1).all() and (d[1500:] == np.float32(10.0)).all()
    far = base[:50] + np.float32(10.5)                              # inside the grid, beyond the cap of 3
    d, i = _index_check(far, base[:50], 3.0)
    assert (i == -1).all() and (d == np.float32(3.0)).all()
    dist, index = pointcloud.nearest_index(_g(q), torch.zeros(0, 3, device=DEV), 7.5)
    assert (dist == 7.5).all() and (index == -1).all() and index.dtype == torch.int32
    dist, index = pointcloud.nearest_index(torch.zeros(0, 3, device=DEV), _g(t), 7.5)
    assert dist.numel() == 0 and index.numel() == 0
    with pytest.raises(ValueError):                                 # a grid without the indices in its w lane
        pointcloud.nearest_index(_g(q), _g(t), 1.0, grid=pointcloud.PointGrid(_g(t), 1.0))


def test_nearest_index_cell_choice_and_ties_across_cells():
    rs = np.random.RandomState(8)
    t = rs.uniform(-50, 50, (20_000, 3)).astype(np.float32)
    q = rs.uniform(-80, 80, (5000, 3)).astype(np.float32)
    # an integer lattice in shuffled order, queried at half-integer offsets: 2, 4 or 8 targets at exactly the same d2, in
    # different cells for the small cell sides; the lowest index must win whichever cell is visited first
    lat = np.stack(np.meshgrid(*[np.arange(12.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    lat = lat[rs.permutation(len(lat))].astype(np.float32)
    ql = (lat[rs.choice(len(lat), 3000)] + rs.choice([0.0, 0.5], (3000, 3))).astype(np.float32)
    for cell in (0.05, 0.7, 3.0, 40.0):
        _index_check(q, t, 30.0, cell=cell)
        _index_check(ql, lat, 30.0, cell=cell)
        _index_check(ql, lat, 0.75, cell=cell)                      # ties right at the cap: 0.75 and sqrt(0.75) > 0.75


# ------------------------------------------------------------------------------------------------------------ pair sums
def _sums_case(m, n, seed, cap=0.05, spread=0.02):
    rs = np.random.RandomState(seed)
    t = rs.uniform(-1, 1, (n, 3)).astype(np.float32) * np.array([2.0, 1.5, 0.3], np.float32) + np.array([1.5, -0.8, 0.6], np.float32)
    T = synth.similarity(0.7, (0.2, 0.4, 1.0), (0.004, -0.003, 0.002), 1.003, about=(1.5, -0.8, 0.6))
    inv = np.linalg.inv(T)
    s = t[rs.choice(n, m)].astype(np.float64) + rs.randn(m, 3) * spread
    return (s @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32), t, T, cap


def _check_sums(s, t, T, cap, order=None):
    p = R.transform(s, T)
    _, idx = R.nearest_index(p, t, cap)
    hit = idx >= 0
    terms = R.pair_terms(p[hit], t[idx[hit]])
    want = R.sum_terms(terms)
    got, dist, index = tt_eval.pair_sums(_g(s), T, _g(t), cap, order=order, return_pairs=True)
    got = got.cpu().numpy()
    assert got.shape == (R.N_SUMS,) and got[0] == hit.sum() == want[0]
    assert np.array_equal(index.cpu().numpy(), idx)
    # every term is exact in float64 (the |p - q|^2 and |p|^2 terms are the same three products in the same order on both
    # sides): only the order of the n additions differs, each within 2^-53 of the running sum
    bound = 2.0 * max(len(terms), 1) * 2.0 ** -53 * np.abs(terms).sum(0) if len(terms) else np.zeros(R.N_SUMS)
    err = np.abs(got - want)
    assert (err <= bound).all(), (err, bound)
    return got


def test_pair_sums_match_the_reference_on_50000_points():
    s, t, T, cap = _sums_case(50_000, 20_000, 1)
    got = _check_sums(s, t, T, cap)
    assert 0.2 * len(s) < got[0] < 0.999 * len(s)                   # some pairs accepted, some refused
    dev_s, dev_t = _g(s), _g(t)
    assert torch.equal(tt_eval.transform_points(dev_s, T).cpu(), torch.from_numpy(R.transform(s, T)))
    grid = pointcloud.index_grid(dev_t)
    order = torch.sort(grid.keys(tt_eval.transform_points(dev_s, T)), stable=True)[1]
    _check_sums(s, t, T, cap, order=order)                          # cell order: another order of the same terms


def test_pair_sums_are_reproducible_across_runs_and_streams():
    s, t, T, cap = _sums_case(50_000, 20_000, 2)
    dev_s, dev_t = _g(s), _g(t)
    a = tt_eval.pair_sums(dev_s, T, dev_t, cap)
    b = tt_eval.pair_sums(dev_s, T, dev_t, cap)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = tt_eval.pair_sums(dev_s, T, dev_t, cap)
    torch.cuda.current_stream().wait_stream(side)
    assert a[0] > 1000 and torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("m", [1, 255, 257, 1000, _lib.ICP_MAX_GROUPS * 256 + 1])
def test_pair_sums_edge_sizes(m):
    """257: the second workgroup holds one point; MAX_GROUPS * 256 + 1: one lane takes a second point (a wrong record count
    in the reduce pass shows at both)."""
    s, t, T, cap = _sums_case(m, 64, 3 + m % 7, cap=0.08)
    got = _check_sums(s, t, T, cap)
    assert got[0] > 0


def test_pair_sums_without_an_accepted_pair():
    s, t, T, cap = _sums_case(700, 500, 5)
    got, dist, index = tt_eval.pair_sums(_g(s + np.float32(50.0)), T, _g(t), cap, return_pairs=True)
    assert (got == 0).all() and (index == -1).all() and (dist == np.float32(cap)).all()
    T_icp, fit, rmse, it = tt_eval.icp(_g(s + np.float32(50.0)), _g(t), cap)
    assert np.array_equal(T_icp, np.eye(4)) and fit == 0.0 and rmse == 0.0 and it == 0       # fewer than 3 pairs: T unchanged


# ----------------------------------------------------------------------------------------------------------- voxel mean
def _voxel_cases():
    rs = np.random.RandomState(13)
    v = 0.25
    lo = np.array([-1.0, 2.0, 0.5])
    o = (lo - 0.5 * v).astype(np.float32).astype(np.float64)
    faces = o + v * rs.randint(1, 9, (400, 3))                                  # exactly on voxel faces o + k v
    faces = np.concatenate([lo[None], faces])
    surf = synth.make_tt_scene(n_gt=200_000, n_pred=10, tau=0.01, seed=2)["gt"]
    surf = surf + rs.randn(*surf.shape).astype(np.float32) * 0.002
    return {"faces": (faces, v), "negative": (rs.uniform(-7, -3, (3000, 3)), 0.3),
            "one_voxel": (rs.uniform(0.01, 0.09, (500, 3)) + 4.0, 0.5), "one_per_voxel": (rs.permutation(64)[:, None] * 1.0 + rs.uniform(0.2, 0.3, (64, 3)), 0.5),
            "single": (np.array([[1.0, -2.0, 3.0]]), 0.1), "duplicates": (np.repeat(rs.uniform(-1, 1, (50, 3)), 7, 0), 0.05),
            "surface": (surf, 0.01)}


@pytest.mark.parametrize("case", ["faces", "negative", "one_voxel", "one_per_voxel", "single", "duplicates", "surface"])
def test_voxel_down_sample_matches_the_reference(case):
    pts, v = _voxel_cases()[case]
    pts = np.asarray(pts, np.float32)
    want, wkeys, wcounts = R.voxel_down_sample(pts, v)
    got, keys, counts = tt_eval.voxel_down_sample(_g(pts), v, return_info=True)
    assert np.array_equal(keys.cpu().numpy(), wkeys) and np.array_equal(counts.cpu().numpy(), wcounts)   # same voxels, same order
    assert (np.diff(wkeys) > 0).all() and int(wcounts.sum()) == len(pts)
    ok = _ulp_close(got.cpu().numpy(), want, ulps=1)
    assert ok.all(), (case, int((~ok).sum()))
    if case == "one_voxel":
        assert len(want) == 1
    if case == "one_per_voxel":
        assert len(want) == 64 and np.array_equal(np.sort(got.cpu().numpy(), 0), np.sort(pts, 0))
    if case == "duplicates":
        assert (wcounts % 7 == 0).all()
    if case == "surface":
        assert 20_000 < len(want) < 190_000 and wcounts.max() > 3
    assert torch.equal(got, tt_eval.voxel_down_sample(_g(pts), v))


def test_voxel_down_sample_empty_and_bad_arguments():
    assert tt_eval.voxel_down_sample(torch.zeros(0, 3, device=DEV), 0.1).shape == (0, 3)
    with pytest.raises(ValueError):
        tt_eval.voxel_down_sample(torch.zeros(4, 3, device=DEV), 0.0)
    with pytest.raises(ValueError):                                  # more voxels along an axis than a key can address
        tt_eval.voxel_down_sample(_g(np.array([[0.0, 0, 0], [1e4, 0, 0]])), 1e-3)


# ----------------------------------------------------------------------------------------------------------------- crop
def _polygons():
    a = np.linspace(0, 2 * np.pi, 10, endpoint=False)
    star = np.stack([np.cos(a), np.sin(a)], 1) * np.where(np.arange(10) % 2 == 0, 1.9, 0.8)[:, None]
    b = np.linspace(0, 2 * np.pi, 64, endpoint=False)
    gon = np.stack([1.7 * np.cos(b), 1.3 * np.sin(b)], 1)
    return {"triangle": np.array([[-1.5, -1.2], [1.8, -0.4], [-0.2, 1.6]]),
            "L": np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 0.0], [0.0, 0.0], [0.0, 1.0], [-1.0, 1.0]]),
            "star": star, "64-gon": gon}


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
@pytest.mark.parametrize("shape", ["triangle", "L", "star", "64-gon"])
def test_crop_matches_the_reference(axis, shape):
    rs = np.random.RandomState(len(shape) + ord(axis))
    iu, iv, iw = R._UV[axis]
    poly2 = _polygons()[shape] + np.array([0.3, -0.2])
    poly = np.zeros((len(poly2), 3))
    poly[:, iu], poly[:, iv] = poly2[:, 0], poly2[:, 1]
    poly[:, iw] = rs.uniform(-9, 9, len(poly2))                       # the polygon's own coordinate along the axis is ignored
    crop = {"orthogonal_axis": axis, "axis_min": -0.5, "axis_max": 0.75, "bounding_polygon": poly}
    pts = rs.uniform(-2.2, 2.2, (100_000, 3))
    pts[:, iw] = rs.uniform(-1.0, 1.2, len(pts))
    k = len(poly2)
    pts[:5000, iv] = np.float32(poly2[rs.randint(0, k, 5000), 1])     # v equal to a vertex's (as the float32 the kernel reads)
    pts[5000:6000, iu] = np.float32(poly2[rs.randint(0, k, 1000), 0])
    pts[6000:7000, iw] = -0.5                                         # exactly at axis_min / axis_max: kept when inside
    pts[7000:8000, iw] = 0.75
    pts[8000:8200, iw] = np.nextafter(np.float32(0.75), np.float32(1))
    pts[8200:8400, iw] = np.nextafter(np.float32(-0.5), np.float32(-1))
    pts[8400:8400 + k] = poly + np.array([0.0, 0.0, 0.0])             # the vertices themselves
    pts = pts.astype(np.float32)
    want = R.crop_mask(pts, crop)
    got = tt_eval.crop_points(_g(pts), crop)
    assert got.dtype == torch.bool and torch.equal(got.cpu(), torch.from_numpy(want))
    assert 0.05 < want.mean() < 0.6
    assert want[6000:8000].any() and not want[8000:8400].any()
    in_range = (pts[:, iw] >= -0.5) & (pts[:, iw] <= 0.75)
    flat = dict(crop, axis_min=-100.0, axis_max=100.0)
    assert np.array_equal(want, R.crop_mask(pts, flat) & in_range)    # the bounds at axis_min / axis_max are inclusive


def test_crop_empty_and_bad_polygons():
    crop = {"orthogonal_axis": "Z", "axis_min": 0.0, "axis_max": 1.0, "bounding_polygon": np.zeros((3, 3))}
    assert tt_eval.crop_points(torch.zeros(0, 3, device=DEV), crop).numel() == 0
    for p in (2, _lib.CROP_MAX_VERTICES + 1):
        with pytest.raises(ValueError):
            tt_eval.crop_points(torch.zeros(4, 3, device=DEV), dict(crop, bounding_polygon=np.zeros((p, 3))))
    big = np.zeros((_lib.CROP_MAX_VERTICES, 3))
    a = np.linspace(0, 2 * np.pi, len(big), endpoint=False)
    big[:, 0], big[:, 1] = np.cos(a), np.sin(a)
    pts = np.random.RandomState(0).uniform(-1.2, 1.2, (20_000, 3)).astype(np.float32)
    c = dict(crop, axis_min=-2.0, axis_max=2.0, bounding_polygon=big)
    assert torch.equal(tt_eval.crop_points(_g(pts), c).cpu(), torch.from_numpy(R.crop_mask(pts, c)))


# ------------------------------------------------------------------------------------------------------ ICP, exact pairs
def _exact_case(with_scaling):
    """A jittered 70 x 70 grid surface (spacing 0.05, jitter +-0.01) and its fp32-rounded inverse image under a known
    similarity (0.2 degrees, 5e-3 translation, scale 1.001): the largest displacement is 0.011, well below half the
    smallest spacing, so every nearest neighbour is the true partner from the first iteration."""
    rs = np.random.RandomState(12)
    g = (np.arange(70) - 34.5) * 0.05
    x, y = [a.reshape(-1) + rs.uniform(-0.01, 0.01, 4900) for a in np.meshgrid(g, g, indexing="ij")]
    z = 0.3 * np.sin(1.3 * x) * np.cos(0.9 * y) + rs.uniform(-0.01, 0.01, 4900)
    target = np.stack([x, y, z], 1).astype(np.float32)
    M = synth.similarity(0.2, (0.3, -0.5, 0.8), np.array([0.6, -0.48, 0.64]) * 5e-3, 1.001 if with_scaling else 1.0)
    inv = np.linalg.inv(M)
    source = (target.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return source, target, M


@pytest.mark.parametrize("with_scaling", [True, False])
def test_icp_recovers_a_known_transform_from_exact_pairs(with_scaling):
    source, target, M = _exact_case(with_scaling)
    assert np.linalg.norm(source.astype(np.float64) - target, axis=1).max() < 0.0115
    _, index = pointcloud.nearest_index(_g(source), _g(target), 0.02)
    assert torch.equal(index.cpu(), torch.arange(4900, dtype=torch.int32))
    T, fit, rmse, it = tt_eval.icp(_g(source), _g(target), 0.02, with_scaling=with_scaling)
    err = np.abs(T - M).max()
    print(f"\nexact pairs (with_scaling={with_scaling}): max entry error {err:.3e}, fitness {fit}, rmse {rmse:.3e}, {it} iterations")
    # one unaveraged fp32 rounding of a coordinate of this extent is ~2e-7: 1e-6 is a cap, not a measurement
    assert err < 1e-6
    assert it <= 3 and fit == 1.0
    assert np.array_equal(T[3], [0, 0, 0, 1])
    if not with_scaling:
        assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12
    Tr, _, _, itr = R.icp(source, target, 0.02, with_scaling=with_scaling)
    assert it == itr and np.abs(T - Tr).max() < 1e-9
    # from a given start, and limited to one iteration
    T1, _, _, it1 = tt_eval.icp(_g(source), _g(target), 0.02, max_iter=1, with_scaling=with_scaling, init=np.eye(4))
    assert it1 == 1 and np.abs(T1 - M).max() < 1e-6


# ---------------------------------------------------------------------------------------------------- noisy scene, shared
SCENE_SEED = 0


@functools.lru_cache(None)
def _scene():
    return synth.make_tt_scene(n_gt=30_000, n_pred=30_000, tau=0.01, seed=SCENE_SEED)


@functools.lru_cache(None)
def _ref_forward():
    sc = _scene()
    return R.evaluate(sc["pred"], sc["gt"], sc["crop"], sc["trans"], sc["tau"])


@functools.lru_cache(None)
def _ref_reversed_register():
    sc = _scene()
    return R.register(sc["pred"], sc["gt"], sc["crop"], sc["trans"], sc["tau"], reverse=True)


def test_icp_on_a_noisy_scene_matches_the_reference():
    sc = _scene()
    tau = sc["tau"]
    s = R.transform(sc["pred"], sc["trans"])
    s = R.voxel_down_sample(s[R.crop_mask(s, sc["crop"])], tau)[0]
    t = R.voxel_down_sample(sc["gt"][R.crop_mask(sc["gt"], sc["crop"])], tau)[0]
    Tf, ff, rf, itf = R.icp(s, t, 20 * tau)
    Tb, _, _, itb = R.icp(s, t, 20 * tau, reverse=True)
    assert itf == itb, "the reference's two summation orders disagree on this scene: choose another seed"
    order_effect = np.abs(Tf - Tb).max()
    tol = max(10.0 * order_effect, 1e-9)
    T, fit, rmse, it = tt_eval.icp(_g(s), _g(t), 20 * tau)
    diff = np.abs(T - Tf).max()
    print(f"\nnoisy icp ({len(s)} -> {len(t)} points): {it} iterations; reference forward vs reversed order {order_effect:.3e}, "
          f"GPU vs reference {diff:.3e} (allowed {tol:.3e}); fitness {fit:.6f} rmse {rmse:.6e}")
    assert it == itf
    assert diff <= tol
    assert abs(fit - ff) <= 1.0 / len(s) and abs(rmse - rf) <= 1e-9


def test_register_on_a_noisy_scene_matches_the_reference():
    sc = _scene()
    want = _ref_forward()
    Tb, its_b = _ref_reversed_register()
    assert want["iterations"] == its_b, "the reference's two summation orders disagree on this scene: choose another seed"
    order_effect = np.abs(want["transform"] - Tb).max()
    tol = max(10.0 * order_effect, 1e-9)
    info = {}
    T = tt_eval.register(_g(sc["pred"]), _g(sc["gt"]), sc["crop"], sc["trans"], sc["tau"], info=info)
    its = [r["iterations"] for r in info["rounds"]]
    diff = np.abs(T - want["transform"]).max()
    print(f"\nregister: iterations per round {its}; reference forward vs reversed order {order_effect:.3e}, "
          f"GPU vs reference {diff:.3e} (allowed {tol:.3e})")
    assert its == want["iterations"]
    assert diff <= tol
    # the registration undoes most of the misalignment the scene was given
    p = sc["pred"].astype(np.float64)

    def rms_off_truth(M):
        d = (p @ M[:3, :3].T + M[:3, 3]) - (p @ sc["true_trans"][:3, :3].T + sc["true_trans"][:3, 3])
        return float(np.sqrt((d * d).sum(1).mean()))
    assert rms_off_truth(sc["trans"]) > sc["tau"] and rms_off_truth(T) < 0.5 * rms_off_truth(sc["trans"])


# ----------------------------------------------------------------------------------------------------------- end to end
def _write_scene(tmp_path, name, sc):
    data, out = tmp_path / "data", tmp_path / "out"
    _tt_layout(data, name, sc)
    out.mkdir(exist_ok=True)
    fusion.write_ply(str(out / f"{name}.ply"), sc["pred"], np.zeros_like(sc["pred"], np.uint8))
    return data, out


def test_cli_matches_the_reference_end_to_end(tmp_path, capsys):
    sc = _scene()
    tau = sc["tau"]
    assert tau == tt_eval.TAU["Barn"]
    data, out = _write_scene(tmp_path, "Barn", sc)
    res = tt_eval.main(["--datapath", str(data), "--plydir", str(out), "--scenes", "Barn", "--json", str(tmp_path / "r.json")])
    printed = capsys.readouterr().out
    assert "Barn: precision" in printed and "mean over 1 scenes" in printed
    got = json.load(open(tmp_path / "r.json"))["scenes"]["Barn"]
    want = _ref_forward()
    for k in ("n_pred_cropped", "n_gt_cropped", "n_pred_sampled", "n_gt_sampled"):
        assert got[k] == want[k], k
    assert got["n_pred"] == len(sc["pred"]) and got["n_gt"] == len(sc["gt"])
    # a distance within a few ulp of tau may fall on the other side of it: at most k such points per direction
    for side, d in (("precision", want["d1"]), ("recall", want["d2"])):
        k = int((np.abs(d.astype(np.float64) - tau) <= 4 * np.spacing(np.float32(tau))).sum())
        assert k <= 1e-3 * len(d)
        assert abs(got[side] - want[side]) <= k / len(d), (side, got[side], want[side], k)
    p, r = got["precision"], got["recall"]
    assert got["fscore"] == pytest.approx(2 * p * r / (p + r), abs=1e-15)
    assert res["mean"]["fscore"] == got["fscore"] and [x["iterations"] for x in got["registration"]] == want["iterations"]
    for name, d, ref_side in (("precision_curve", want["d1"], "precision"), ("recall_curve", want["d2"], "recall")):
        c = np.asarray(got[name])
        assert c.shape == (500,) and (np.diff(c) >= 0).all() and c[-1] <= 1.0
        assert np.abs(c - R.curve(d, tau)).max() <= 2e-3 and abs(c[99] - got[ref_side]) <= 2e-3
    # the scene makes the score informative
    assert 0.2 < want["precision"] < 0.98 and 0.2 < want["recall"] < 0.98
    plain = R.evaluate(sc["pred"], sc["gt"], sc["crop"], sc["trans"], tau, do_register=False)
    assert plain["fscore"] < want["fscore"] - 0.05
    res2 = tt_eval.main(["--datapath", str(data), "--plydir", str(out), "--scenes", "Barn", "--no-register"])
    got2 = res2["scenes"]["Barn"]
    assert got2["registration"] == [] and np.array_equal(np.asarray(got2["transform"]), sc["trans"])
    assert got2["n_pred_sampled"] == plain["n_pred_sampled"]
    assert abs(got2["precision"] - plain["precision"]) <= 1e-3 and got2["fscore"] < got["fscore"] - 0.05
    # --init is right-multiplied onto the scene's transform: trans @ (trans^-1 true_trans) starts at the truth
    init = tmp_path / "init.txt"
    np.savetxt(init, np.linalg.inv(sc["trans"]) @ sc["true_trans"], fmt="%.17g")
    res3 = tt_eval.main(["--datapath", str(data), "--plydir", str(out), "--scenes", "Barn", "--no-register", "--init", str(init)])
    assert np.abs(np.asarray(res3["scenes"]["Barn"]["transform"]) - sc["true_trans"]).max() < 1e-12
    assert res3["scenes"]["Barn"]["fscore"] > got2["fscore"] + 0.05


def test_cli_needs_tau_for_an_unknown_scene_and_scores_it_with_tau(tmp_path):
    sc = synth.make_tt_scene(n_gt=6000, n_pred=5000, tau=0.02, hole_radius=4.0, seed=4)
    data, out = _write_scene(tmp_path, "MyGarden", sc)
    with pytest.raises(SystemExit):
        tt_eval.main(["--datapath", str(data), "--plydir", str(out), "--scenes", "MyGarden"])
    res = tt_eval.main(["--datapath", str(data), "--plydir", str(out), "--scenes", "MyGarden", "--tau", "0.02"])
    assert 0.2 < res["scenes"]["MyGarden"]["fscore"] <= 1.0 and res["scenes"]["MyGarden"]["tau"] == 0.02
    with pytest.raises(FileNotFoundError):
        tt_eval.main(["--datapath", str(data), "--plydir", str(out), "--scenes", "Barn"])


def test_an_empty_crop_scores_zero_without_an_exception():
    sc = synth.make_tt_scene(n_gt=6000, n_pred=5000, tau=0.02, hole_radius=4.0, seed=4)
    crop = dict(sc["crop"], bounding_polygon=np.asarray(sc["crop"]["bounding_polygon"]) + 100.0)
    r = tt_eval.evaluate(_g(sc["pred"]), _g(sc["gt"]), crop, sc["trans"], sc["tau"])
    assert r["fscore"] == 0.0 and r["precision"] == 0.0 and r["recall"] == 0.0
    assert r["n_pred_cropped"] == 0 and r["n_gt_cropped"] == 0 and [x["iterations"] for x in r["registration"]] == [0, 0, 0]
    assert np.array_equal(np.asarray(r["transform"]), sc["trans"])
    # only the prediction empty: recall 0 over a non-empty ground truth
    far = _g(sc["pred"] + np.float32(500.0))
    r = tt_eval.evaluate(far, _g(sc["gt"]), sc["crop"], sc["trans"], sc["tau"], register=False)
    assert r["fscore"] == 0.0 and r["n_pred_cropped"] == 0 and r["n_gt_cropped"] > 0
    assert R.fscore(np.zeros(0), np.ones(5), 0.1) == (0.0, 0.0, 0.0)
