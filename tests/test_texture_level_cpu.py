"""The seam levelling of the texturing stage without a GPU: the numpy restatement of rules L1-L6
(texture_level_ref.py) on hand-made and analytic inputs, what the feature is for, the host solve of rule L3 in
cds_mvsnet_amd/texture.py, and the command lines' errors."""
import numpy as np
import pytest

import render_ref as R
import texture_level_ref as L
import texture_ref as T
from cds_mvsnet_amd import infer, photo_eval, texture


# -------------------------------------------------------------------------------------------------------------------- nodes
def test_nodes_of_two_faces():
    f, view = L.two_faces([1, 1])
    key, cn, corners = L.nodes(f, view, 3)
    assert key.tolist() == [1, 4, 7, 10] and cn.tolist() == [[0, 1, 2], [2, 1, 3]]
    assert corners == [[0], [1, 4], [2, 3], [5]]
    f, view = L.two_faces([2, 0])
    key, cn, corners = L.nodes(f, view, 3)
    assert key.tolist() == [2, 3, 5, 6, 8, 9]                        # vertex 1 and vertex 2 carry both labels, 0 before 2
    assert cn.tolist() == [[0, 2, 4], [3, 1, 5]] and corners == [[0], [4], [1], [3], [2], [5]]
    assert L.vertex_groups(key, 3) == [[0], [1, 2], [3, 4], [5]]
    key, cn, corners = L.nodes(*L.two_faces([-1, 2]), 3)
    assert key.tolist() == [5, 8, 11] and cn.tolist() == [[-1, -1, -1], [1, 0, 2]] and corners == [[4], [3], [5]]
    key, cn, corners = L.nodes(*L.two_faces([-1, -1]), 3)
    assert len(key) == 0 and (cn == -1).all() and corners == []


# ----------------------------------------------------------------------------------------------------------------- no seams
@pytest.mark.parametrize("name,n_views", [("plane", 1), ("sphere", 1), ("clutter", 3)])
def test_without_seams_nothing_changes(name, n_views):
    """One label in use: no pairs, offsets 0, g exactly 0 and the atlas of the unlevelled rule in every byte."""
    base = T.reference(name, n_views)
    assert len(np.unique(base["view"][base["view"] >= 0])) == 1
    out = L.reference(name, n_views, 7)
    lv = out["level"]
    assert len(lv["node_key"]) > 0 and int(lv["table"][:, :, 0].sum()) == 0
    assert not lv["offsets"].any() and not lv["g"].any()
    assert np.array_equal(out["atlas"], base["atlas"])


# ------------------------------------------------------------------------------------------------------- what it is for
ITER = 20


def _plane(iters, **kw):
    v, vc, f, images, shifted, cams = L.plane_setup()
    base = T.texture(v, vc, f, shifted, cams)
    return base, L.level(v, vc, f, shifted, cams, iters, base=base, keep=(0,), **kw)


def test_levelling_removes_the_exposure_steps():
    """plane_mesh(9) reversed (128 faces), three cameras at 128 x 96, the analytic pattern with +0 / +25 / -20 levels per view.
    Measured: jump at the 31 seam pairs 30.20 unlevelled, 0.28 after the per-view offsets, 0.04 after 20 iterations; rms error
    against the pattern (per-channel mean removed) 11.63 unlevelled, 0.88 levelled, 0.88 for the atlas of the images without
    offsets."""
    v, vc, f, images, shifted, cams = L.plane_setup()
    assert len(f) == 128 and shifted.shape == (3, 96, 128, 3)
    base, out = _plane(ITER)
    lv = out["level"]
    assert len(np.unique(base["view"])) == 3 and (base["view"] >= 0).all()
    jump = {}
    for what, g in (("unlevelled", np.zeros_like(lv["g"])), ("offsets only", lv["g_at"][0]), ("levelled", lv["g"])):
        pairs, jump[what] = L.seam_jump(lv["sample"], lv["ok"], lv["node_key"], 3, g)
    rms = {"unlevelled": L.pattern_rms(v, f, base), "levelled": L.pattern_rms(v, f, out),
           "no offsets in the images": L.pattern_rms(v, f, T.texture(v, vc, f, images, cams))}
    print(f"{pairs} seam pairs, mean jump: " + ", ".join(f"{k} {x:.3f}" for k, x in jump.items()))
    print("rms error against the pattern: " + ", ".join(f"{k} {x:.3f}" for k, x in rms.items()))
    assert pairs > 0 and jump["levelled"] <= 0.1 * jump["unlevelled"]
    assert rms["levelled"] <= 0.25 * rms["unlevelled"] and rms["levelled"] <= 2.0 * rms["no offsets in the images"]
    for k in ("uv", "view", "cell"):
        assert np.array_equal(out[k], base[k])


def test_both_steps_matter():
    """The same set-up levelled without rule L3 (offsets forced to 0) at the same ITER: measured rms 2.87 against 0.88."""
    v, vc, f, images, shifted, cams = L.plane_setup()
    _, with_l3 = _plane(ITER)
    _, without = _plane(ITER, force_offsets=np.zeros((3, 3)))
    a, b = L.pattern_rms(v, f, with_l3), L.pattern_rms(v, f, without)
    print(f"rms error with the per-view offsets {a:.3f}, without {b:.3f}")
    assert b > a


def test_many_iterations_stay_finite_and_do_not_widen_the_seams():
    """The sphere under 9 noise views: a vertex carries up to 6 labels, 505 seam pairs; the noise drives |g| past 100, so the
    clamp of rule L6 is at work."""
    out = L.reference("sphere", 9, 200, keep=(0,))
    lv = out["level"]
    groups = L.vertex_groups(lv["node_key"], 9)
    pairs, first = L.seam_jump(lv["sample"], lv["ok"], lv["node_key"], 9, lv["g_at"][0])
    _, last = L.seam_jump(lv["sample"], lv["ok"], lv["node_key"], 9, lv["g"])
    print(f"{len(lv['node_key'])} nodes, up to {max(len(g) for g in groups)} labels at a vertex, {pairs} seam pairs: jump {first:.2f} "
          f"after 0 iterations, {last:.2f} after 200, max |g| {np.abs(lv['g']).max():.1f}")
    assert max(len(g) for g in groups) == 6 and pairs == 505 and pairs == int(lv["table"][:, :, 0].sum())
    assert np.isfinite(lv["g"]).all() and last <= first
    assert np.abs(lv["g"]).max() > 100
    base = T.reference("sphere", 9)
    changed = (out["atlas"] != base["atlas"]).any(2)
    assert changed.any() and (out["atlas"][changed] == 0).any() and (out["atlas"][changed] == 255).any()


# ------------------------------------------------------------------------------------------------------------------ offsets
@pytest.mark.parametrize("name,n_views", [("sphere", 9), ("sphere", 3), ("wild", 3)])
def test_offsets_equal_a_least_squares_statement(name, n_views):
    lv = L.reference(name, n_views, 0)["level"]
    want, M = L.offsets_lstsq(lv["table"], lv["node_key"], n_views)
    A = M.T @ M
    bound = np.linalg.cond(A) * 2.0 ** -50 * np.abs(want).max()
    n_label = np.bincount(lv["node_key"] % n_views, minlength=n_views)
    lib = texture.level_offsets(lv["table"][:, :, 0], lv["table"][:, :, 1:], n_label)
    err_ref, err_lib = np.abs(lv["offsets"] - want).max(), np.abs(lib - want).max()
    print(f"{name} {n_views}: cond {np.linalg.cond(A):.3g}, max |o| {np.abs(want).max():.3g}, bound {bound:.3g}; restatement off by "
          f"{err_ref:.3g}, texture.level_offsets by {err_lib:.3g}")
    assert np.abs(want).max() > 0 and err_ref <= bound and err_lib <= bound


def test_offsets_of_one_pair_split_the_difference():
    table = np.zeros((2, 2, 4), np.int64)
    table[0, 1] = (4, 4 * 256 * 10, 0, -4 * 256 * 6)                 # view 0 is 10 levels brighter in red, 6 darker in blue
    o = texture.level_offsets(table[:, :, 0], table[:, :, 1:], np.array([7, 9]))
    # the ridge costs 2^-10 (7 o_0^2 + 9 o_1^2): it moves the difference by less than 0.01 level and fixes the common level
    assert np.allclose(o[0] - o[1], (-10, 0, 6), atol=0.02) and np.allclose(7 * o[0] + 9 * o[1], 0, atol=1e-9)
    assert not texture.level_offsets(np.zeros((3, 3), np.int64), np.zeros((3, 3, 3), np.int64), np.zeros(3, np.int64)).any()


# ------------------------------------------------------------------------------------------------------------ command lines
BASE = ["--testpath", "a", "--testlist", "b", "--outdir", "c"]
MESH = ["--fuse", "--mesh_voxel", "2"]


@pytest.mark.parametrize("argv,word", [
    (MESH + ["--texture_level", "3"], "belong to --texture"),
    (MESH + ["--texture_level_lambda", "0.5"], "belong to --texture"),
    (MESH + ["--texture", "--texture_level_lambda", "0.5"], "--texture_level ITER"),
    (MESH + ["--texture", "--texture_level", "0", "--texture_level_lambda", "0.5"], "--texture_level ITER"),
    (MESH + ["--texture", "--texture_level", "-1"], "level"),
    (MESH + ["--texture", "--texture_level", "3", "--texture_level_lambda", "0"], "level_lambda"),
    (MESH + ["--texture", "--texture_level", "3", "--texture_level_lambda", "nan"], "level_lambda"),
    (MESH + ["--texture", "--texture_level", "3", "--texture_level_lambda", "inf"], "level_lambda"),
    (MESH + ["--photo_eval", "--texture_level", "-2"], "level"),
])
def test_infer_refuses_level_options_that_do_not_fit(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        infer.parse_args(BASE + argv)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_infer_accepts_level_options():
    args = infer.parse_args(BASE + MESH + ["--texture", "--texture_level", "5"])
    assert args.texture_kw == dict(scale=1.0, max_cell=256, max_size=16384, min_px=1, level=5, level_lambda=0.1)
    args = infer.parse_args(BASE + MESH + ["--photo_eval", "--texture_level", "5", "--texture_level_lambda", "0.25"])
    assert args.texture_kw["level"] == 5 and args.texture_kw["level_lambda"] == 0.25
    args = infer.parse_args(BASE + MESH + ["--texture", "--texture_level", "0"])
    assert args.texture_kw["level"] == 0
    assert "level" not in infer.parse_args(BASE + MESH + ["--texture"]).texture_kw


@pytest.mark.parametrize("main", [texture.main, photo_eval.main])
@pytest.mark.parametrize("argv,word", [(["--texture_level", "-1"], "level"), (["--texture_level_lambda", "0.5"], "--texture_level ITER"),
                                       (["--texture_level", "2", "--texture_level_lambda", "-1"], "level_lambda"),
                                       (["--texture_level", "x"], "invalid int")])
def test_command_lines_refuse_level_values_outside_their_range(main, argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        main(BASE + argv)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_library_call_checks_level_before_the_device():
    v, c, f, images, cams = T.case("plane", 2)
    import torch
    mesh = {"vertices": torch.from_numpy(v), "colors": torch.from_numpy(c), "faces": torch.from_numpy(f)}
    ti, tc = torch.from_numpy(images), torch.from_numpy(cams)
    for bad in (dict(level=-1), dict(level=1.5), dict(level=2, level_lambda=0.0), dict(level=2, level_lambda=float("nan")),
                dict(level=0, level_lambda=float("inf"))):
        with pytest.raises(ValueError, match="level"):
            texture.texture_mesh(mesh, ti, tc, **bad)
    with pytest.raises(ValueError, match="level"):
        texture.texture_scan("nowhere", "none.ply", "nowhere", "none", level=-3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        texture.texture_mesh(mesh, ti, tc, level=3)
    assert texture.LEVEL_MAX_VIEWS == 512 and texture.DEFAULTS["level"] == 0 and texture.DEFAULTS["level_lambda"] == 0.1


def test_format_texture_appends_the_seam_line():
    info = {"H": 8, "W": 16, "faces": 4, "unseen": 1, "units": (6, 8), "views": 3}
    plain = texture.format_texture(info)
    assert "seam" not in plain
    line = texture.format_texture(dict(info, seam=(31, 30.2, 0.04)))
    assert line.startswith(plain) and "31 seam pairs" in line and "30.20 -> 0.04" in line
