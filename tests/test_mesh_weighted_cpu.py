"""The numpy restatement of the weighted integration rule (mesh_weighted_ref.py) against mesh_ref.py, against the
analytic sphere and plane, and at the edges of the rule.  No GPU: the kernels are compared with this restatement in
test_mesh_weighted_gpu.py."""
import numpy as np
import pytest

import cloud_ref as C
import mesh_ref as M
import mesh_weighted_ref as W


# ------------------------------------------------------------------------------------------------- 1. the unweighted rule
@pytest.mark.parametrize("ones", [False, True])
def test_weights_of_one_are_the_unweighted_rule(ones):
    """weights = None and weights = 1 everywhere, no interpolation: sum and n have the bits of mesh_ref.integrate, wn = n."""
    sc, want = M.integration_case(33, 4.0)
    vol = W.allocate(sc["points"], sc["voxel"], 4.0 * sc["voxel"])
    W.integrate(vol, sc["depths"], sc["masks"], sc["images"], sc["cams"], np.ones(sc["depths"].shape, np.uint8) if ones else None)
    assert want["n"].max() > 1
    for name in ("sum", "n", "nc", "rgb"):
        assert np.array_equal(vol[name].view(np.int32), want[name].view(np.int32)), name
    assert np.array_equal(vol["wn"], vol["n"])
    assert np.array_equal(W.extract(vol, 2)["vertices"].view(np.int32), M.extract(want, 2)["vertices"].view(np.int32))


# ------------------------------------------------------------------------------------------------------------ 2. the sphere
def test_sphere_error_by_mode():
    """The 26-camera sphere of mesh_ref.sphere_scene (48 x 48 maps, T = 2.5 voxels, min_weight 2), weights from the normals of
    cloud_ref.depth_normals, jump 0.05.  Every mode gives a closed surface, and the radial error of the vertices falls: angle +
    interp to at most 0.5 x the rms of the unweighted rule, angle alone to at most 0.6 x, the largest error of angle + interp
    below the unweighted one.  Measured (voxels, rms / max): one 0.1048 / 0.4067, interp 0.1033 / 0.3702, angle 0.0364 / 0.1789,
    angle + interp 0.0226 / 0.1643; 69 % of the kept pixels have a normal."""
    sc, _, plain = M.sphere_case()
    share = W.sphere_weights()[1]
    err = {}
    for weighted in (False, True):
        for interp in (False, True):
            vol, mesh = W.sphere_mode(weighted, interp)
            tp = M.topology(mesh["faces"], len(mesh["vertices"]))
            assert tp["euler"] == 2 and (tp["edge_uses"] == 2).all() and tp["directed_unique"] and tp["reverse_present"]
            assert tp["used_vertices"] == len(mesh["vertices"])
            err[weighted, interp] = W.radial_error(mesh["vertices"], sc)
            print(f"angle weights {weighted}, interp {interp}: rms {err[weighted, interp][0]:.4f}, max {err[weighted, interp][1]:.4f} "
                  f"voxels; {len(mesh['vertices'])} vertices, {len(mesh['faces'])} faces")
    print(f"{100 * share:.1f} % of the kept pixels have a normal")
    assert np.array_equal(W.sphere_mode(False, False)[1]["vertices"].view(np.int32), plain["vertices"].view(np.int32))
    base = err[False, False]
    assert err[True, True][0] <= 0.5 * base[0]
    assert err[True, False][0] <= 0.6 * base[0]
    assert err[True, True][1] < base[1]


# ------------------------------------------------------------------------------------------------------- 3. plane exactness
def test_interpolation_is_exact_on_a_plane():
    """1 / z is affine in the pixel for a plane: on cloud_ref.tilted_plane rounded to fp32 the interpolated depth is within 2^-22
    (relative) of the plane's depth at the sub-pixel position.  Each fp32 depth is off by at most 2^-24, a convex combination of
    their inverses by no more; the bar leaves a factor of four."""
    h, w = 37, 50
    depth, K, _, _ = C.tilted_plane(h, w, np.float32)
    n = np.array([0.1, -0.07, 1.0])
    rs = np.random.RandomState(7)
    u, v = rs.uniform(0.5, w - 0.5, 4000), rs.uniform(0.5, h - 0.5, 4000)
    u[:4], v[:4] = [0.5, 1.5, w - 1.0, 7.25], [0.5, h - 1.0, 3.5, 9.75]            # on pixel centres and on quad edges
    dd, took = W.interp_depth(depth, np.ones((h, w), np.uint8), u, v, W.JUMP)
    assert took.all()
    want = n[2] * 650.0 / (n @ (np.linalg.inv(K) @ np.stack([u, v, np.ones_like(u)])))
    rel = np.abs(dd - want) / want
    near = np.abs(depth[np.floor(v).astype(int), np.floor(u).astype(int)] - want) / want
    print(f"largest relative error {rel.max():.3g} = 2^{np.log2(rel.max()):.1f} (the nearest pixel's depth: {near.max():.3g})")
    assert rel.max() <= 2.0 ** -22
    assert near.max() > 1e-5                                                        # the plane is tilted: there is something to gain


# ------------------------------------------------------------------------------------------------------------ 4. fallbacks
def _map(h=6, w=7):
    rs = np.random.RandomState(3)
    return (10.0 + 0.05 * rs.rand(h, w)).astype(np.float32), np.ones((h, w), np.uint8)


def _nearest_bits(depth, mask, u, v, jump=W.JUMP):
    u, v = np.atleast_1d(np.asarray(u, np.float64)), np.atleast_1d(np.asarray(v, np.float64))
    dd, took = W.interp_depth(depth, mask, u, v, jump)
    near = depth[np.floor(v).astype(int), np.floor(u).astype(int)].astype(np.float64)
    return ~took & (dd.view(np.int64) == near.view(np.int64)), took


@pytest.mark.parametrize("bad", ["mask", np.nan, 0.0, -2.0, np.inf])
def test_a_quad_with_a_corner_that_is_not_kept_takes_the_nearest_pixel(bad):
    depth, mask = _map()
    if bad == "mask":
        mask[2, 3] = 0
    else:
        depth[2, 3] = bad
    # a position in each of the four quads that hold pixel (x 3, y 2), next to another (kept) pixel
    u = np.array([2.9, 4.1, 2.9, 4.1])
    v = np.array([1.9, 1.9, 3.1, 3.1])
    fell, took = _nearest_bits(depth, mask, u, v)
    assert fell.all() and not took.any()
    _, took = _nearest_bits(depth, mask, u - 1.5, v)                               # the quads one and a half pixels to the left
    assert took[[0, 2]].all()


def test_the_jump_bound_is_inclusive():
    depth, mask = _map()
    jump = 0.25                                                                     # exact in fp32, as are 1 and 1.25
    depth[:] = 1.125
    depth[2, 3], depth[2, 4] = 1.0, 1.25                                            # hi - lo == jump lo
    dd, took = W.interp_depth(depth, mask, [4.0], [2.5], jump)
    assert took.all() and dd[0] == 1.0 / (1.0 + 0.5 * (0.8 - 1.0))
    depth[2, 4] = np.nextafter(np.float32(1.25), np.float32(2))
    fell, took = _nearest_bits(depth, mask, [3.9, 4.1], [2.4, 2.6], jump)
    assert fell.all()
    depth[2, 4], depth[2, 3] = 1.25, np.nextafter(np.float32(1.0), np.float32(0))   # a smaller lo lowers the bound as well
    assert _nearest_bits(depth, mask, [3.9], [2.4], jump)[0].all()


def test_quads_cut_by_the_border_take_the_nearest_pixel():
    depth, mask = _map()
    h, w = depth.shape
    u = np.array([0.0, 0.49, w - 0.4, w - 1e-9, 3.2, 3.2, 3.2, 3.2, 0.2, w - 0.2])
    v = np.array([2.2, 2.2, 2.2, 2.2, 0.0, 0.49, h - 0.4, h - 1e-9, 0.3, h - 0.3])
    fell, _ = _nearest_bits(depth, mask, u, v)
    assert fell.all()
    _, took = _nearest_bits(depth, mask, [0.5, w - 0.5 - 1e-9, 3.2, 3.2], [2.2, 2.2, 0.5, h - 0.5 - 1e-9])
    assert took.all()                                                               # the outermost pixel centres are inside
    one_row, took = _nearest_bits(depth[:1], mask[:1], [0.7, 3.5], [0.5, 0.2])       # a map of one row has no quad
    assert one_row.all()


# ---------------------------------------------------------------------------------------------------------- 5. weight rule
def _weight_case():
    h, w = 3, 5
    K = np.array([[40.0, 0.5, 2.5], [0.0, 30.0, 1.5], [0.0, 0.0, 1.0]])            # pixel (x 2, y 1) lies on the axis
    E = np.eye(4)
    E[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]                                 # 90 degrees about z
    E[:3, 3] = [3.0, -2.0, 5.0]
    return h, w, K, E, np.full((h, w), 7.0, np.float32), np.ones((h, w), np.uint8)


def _normals(h, w, E, cam_normal):
    """A world-frame normal field whose camera-frame value is ``cam_normal`` everywhere."""
    nw = E[:3, :3].T @ np.asarray(cam_normal, np.float64)
    return np.broadcast_to(nw.astype(np.float32)[:, None, None], (3, h, w)).copy(), np.ones((h, w), np.uint8)


def test_weight_rule_angle_term():
    h, w, K, E, depth, mask = _weight_case()
    nrm, ok = _normals(h, w, E, (0.0, 0.0, -1.0))                                   # faces the camera along the axis
    got = W.view_weights(depth, mask, K, E, nrm, ok)
    assert got[1, 2] == 255 and got.min() >= 1
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    rays = np.linalg.inv(K) @ np.stack([xs, ys, np.ones_like(xs)]).reshape(3, -1)   # an independent route to the cosine
    cos = (rays[2] / np.linalg.norm(rays, axis=0)).reshape(h, w)
    assert np.abs(got.astype(np.float64) - 255.0 * cos).max() <= 0.5 + 1e-9
    s = np.sqrt(0.75)
    got = W.view_weights(depth, mask, K, E, *_normals(h, w, E, (s, 0.0, -0.5)))      # 60 degrees off the axis
    assert got[1, 2] == 128                                                         # floor(127.5 + 0.5)
    ok0 = ok.copy()
    ok0[0, 1] = 0
    assert W.view_weights(depth, mask, K, E, nrm, ok0)[0, 1] == 1                   # no normal: the minimum
    back = W.view_weights(depth, mask, K, E, *_normals(h, w, E, (0.0, 0.0, 1.0)))
    assert (back == 1).all()                                                        # a back-facing normal: the minimum
    graz = W.view_weights(depth, mask, K, E, *_normals(h, w, E, (1.0, 0.0, 0.0)))
    assert graz[1, 2] == 1 and graz[1, 0] > 1 and graz[1, 4] == 1                  # grazing on the axis, facing left of it only
    nan = nrm.copy()
    nan[:, 2, 2] = np.nan
    assert W.view_weights(depth, mask, K, E, nan, ok)[2, 2] == 1
    assert (W.view_weights(depth, mask, K, E) == 255).all()                         # normals NULL: a = 1


def test_weight_rule_confidence_and_mask():
    h, w, K, E, depth, mask = _weight_case()
    conf = np.full((h, w), 0.5, np.float32)
    conf[0, 0], conf[0, 1], conf[0, 2], conf[0, 3], conf[0, 4] = np.nan, -0.3, 1.7, 0.0, np.inf
    got = W.view_weights(depth, mask, K, E, conf=conf)
    assert got[0].tolist() == [1, 1, 255, 1, 255] and (got[1:] == 128).all()
    nrm, ok = _normals(h, w, E, (np.sqrt(0.75), 0.0, -0.5))
    both = W.view_weights(depth, mask, K, E, nrm, ok, conf)
    assert both[1, 2] == 64 and both[0, 0] == 1                                     # floor(255 * 0.25 + 0.5)
    assert np.array_equal(W.view_weights(depth, mask, K, E, nrm, ok, None), W.view_weights(depth, mask, K, E, nrm, ok))
    mask[1, 1] = 0
    depth[1, 3], depth[2, 0], depth[2, 1], depth[2, 2] = np.nan, 0.0, -1.0, np.inf
    got = W.view_weights(depth, mask, K, E, nrm, ok, conf)
    assert got[1, 1] == 0 and got[1, 3] == 0 and got[2, :3].tolist() == [0, 0, 0] and got[1, 2] == 64


def test_zero_weight_skips_the_view_and_extract_divides_by_wn():
    sc, wt, vol = W.integration_case(33, 4.0, True, True)
    assert (wt == 0).any() and (vol["wn"] > vol["n"]).any() and (vol["wn"] >= vol["n"]).all()
    assert ((vol["n"] == 0) == (vol["wn"] == 0)).all()
    plain, nearest = M.integration_case(33, 4.0)[1], W.integration_case(33, 4.0, True, False)[2]
    assert (nearest["n"] <= plain["n"]).all() and (nearest["n"] < plain["n"]).any()   # views with weight 0 are not counted
    assert (vol["n"] != nearest["n"]).any()                      # an interpolated depth moves some points across sdf = -T
    mesh = W.extract(vol, 2)
    assert len(mesh["faces"]) > 0 and np.isfinite(mesh["vertices"]).all()


# -------------------------------------------------------------------------------------------------------------- options
def test_command_line_option_errors(tmp_path, capsys):
    from cds_mvsnet_amd import infer, mesh
    base = ["--outdir", str(tmp_path), "--testlist", str(tmp_path / "list.txt")]
    for extra, text in ((["--from_mesh", "x.ply", "--mesh_weight", "angle"], "--mesh_weight"),
                        (["--from_mesh", "x.ply", "--mesh_interp"], "--mesh_interp"),
                        (["--from_mesh", "x.ply", "--mesh_interp_jump", "0.1"], "--mesh_interp_jump"),
                        (["--mesh_interp"], "--mesh_voxel"),
                        (["--testpath", "x", "--mesh_voxel", "1", "--mesh_interp_jump", "0.1"], "belongs to --mesh_interp"),
                        (["--testpath", "x", "--mesh_voxel", "1", "--mesh_interp", "--mesh_interp_jump", "0"], "must be positive"),
                        (["--testpath", "x", "--mesh_voxel", "1", "--mesh_weight", "cosine"], "invalid choice")):
        with pytest.raises(SystemExit):
            mesh.main(base + extra)
        assert text in capsys.readouterr().err, extra
    common = ["--testpath", "x", "--testlist", str(tmp_path / "list.txt"), "--outdir", str(tmp_path)]
    for extra in (["--fuse", "--mesh_weight", "conf"], ["--fuse", "--mesh_interp"]):
        with pytest.raises(SystemExit):
            infer.parse_args(common + extra)
        assert "--mesh_voxel" in capsys.readouterr().err
    args = infer.parse_args(common + ["--fuse", "--mesh_voxel", "2", "--mesh_weight", "angle_conf", "--mesh_interp"])
    assert (args.mesh_weight, args.mesh_interp, args.mesh_interp_jump) == ("angle_conf", True, 0.05)
    assert infer.parse_args(common).mesh_weight == "one"
