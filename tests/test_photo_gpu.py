"""The kernels of csrc/photo.hip against the numpy restatement of their rules (photo_ref.py): the shaded image equal
in every byte, the integer sums and the SSIM map equal in every bit, the SSIM sums within the bound of a sum in any order and the
same bits run to run; and the way from a scan's mesh to its score through the command line and infer --photo_eval."""
import filecmp
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import photo_ref as P
import render_ref as R
import texture_ref as T
from cds_mvsnet_amd import infer, photo_eval, texture
from test_mvs_io import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = P.TILE
assert TILE == photo_eval.TILE
EDGES = [1, 10, 11, 12, TILE + 9, TILE + 10, TILE + 11, 2 * TILE + 10]          # no window, one, one tile and its halo +- 1, two tiles


# --------------------------------------------------------------------------------------------------------------------- shade
def _mesh(v, f):
    return {"vertices": torch.from_numpy(v).cuda(), "faces": torch.from_numpy(np.ascontiguousarray(f)).cuda()}


def _tex(uv, atlas):
    return {"uv": torch.from_numpy(np.ascontiguousarray(uv, np.int32)).cuda(), "atlas": torch.from_numpy(np.array(atlas, np.uint8)).cuda()}


def _same_image(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}, expected {want.dtype} {want.shape}"
    bad = got != want
    assert not bad.any(), f"{what}: differs in {int(bad.sum())} of {bad.size} bytes, first at {np.argwhere(bad)[0].tolist()}"


def _shade_case(name, n_views=1, h=R.H, w=R.W, scale=1.0, max_cell=256, **kw):
    v, c, f, images, cams, face = P.shade_case(name, n_views, h, w)
    tex, want, clamp = P.shade_reference(name, n_views, h, w, scale, max_cell)
    out = photo_eval.shade_views(_mesh(v, f), _tex(tex["uv"], tex["atlas"]), torch.from_numpy(cams), h, w, **kw)
    assert sorted(out) == ["depth", "face", "image", "valid"] and all(t.is_cuda for t in out.values())
    assert np.array_equal(out["face"].cpu().numpy(), face)
    got = out["image"].cpu().numpy()
    print(f"{name}, {n_views} views of {h} x {w}, scale {scale}, max_cell {max_cell}, {kw}: atlas {tex['atlas'].shape[1]} x "
          f"{tex['atlas'].shape[0]}, {int((face >= 0).sum())} pixels hit, {int(want.any(-1).sum())} not black, {int(clamp.sum())} clamped")
    _same_image(got, want, f"{name} {n_views} {h}x{w} {scale} {kw}")
    return got, want, tex, clamp


@pytest.mark.parametrize("name", ["plane", "sphere", "clutter", "wild"])
@pytest.mark.parametrize("n_views", [1, 3])
def test_shade_equals_the_restatement(name, n_views):
    got, want, tex, _ = _shade_case(name, n_views)
    assert want.any()


def test_shade_of_meshes_that_look_at_the_camera():
    """texture_ref's winding: the faces are seen, so the atlas holds image samples and not vertex colours."""
    for name in ("t:plane", "t:wild"):
        got, want, tex, _ = _shade_case(name, 3)
        assert (tex["view"] >= 0).any() and want.any()


@pytest.mark.parametrize("scale", [0.25, 8.0])
def test_shade_smallest_cell_and_clamped_max_cell(scale):
    got, want, tex, _ = _shade_case("sphere", 3, scale=scale, max_cell=16)
    sizes = set(np.unique(tex["cell"][:, 2]).tolist())
    assert sizes == ({4} if scale == 0.25 else {4, 16}), sizes


def test_shade_map_of_50_by_37():
    _shade_case("wild", 2, 37, 50)
    _shade_case("t:wild", 2, 37, 50)
    _shade_case("sphere", 2, 37, 50)


def test_shade_image_one_pixel_wide():
    got, want, _, _ = _shade_case("t:special", 1, R.H, 1)
    assert want.any()


def test_shade_chunk_does_not_change_the_result():
    a, _, _, _ = _shade_case("sphere", 3, chunk=8)
    b, _, _, _ = _shade_case("sphere", 3, chunk=1)
    _same_image(b, a, "chunk 1 against 8")


def test_shade_grazing_pixels_stay_inside_their_cell():
    """The clamp of rule S.  No pixel of wild_mesh() clamps in any view (see photo_ref.grazing_mesh), so the faces seen edge-on are a
    case of their own; wild is still shaded equal above."""
    for scale in (1.0, 8.0):
        got, want, tex, clamp = _shade_case("grazing", 1, scale=scale)
        assert clamp.any() and (tex["view"] >= 0).all()
    _, _, _, clamp = _shade_case("wild", 3)
    print(f"wild, 3 views: {int(clamp.sum())} pixels clamp")


def test_shade_falls_back_to_black_for_cells_outside_the_atlas():
    """Faces whose uv lies beyond the atlas, before it, or gives c < 4: black, and nothing is read out of bounds."""
    v, c, f, images, cams, face = P.shade_case("t:plane", 1)
    tex, plain, _ = P.shade_reference("t:plane", 1)
    uv = tex["uv"].copy()
    seen = [int(k) for k in np.unique(face[face >= 0])]
    far, before, small, big, edge = seen[0], seen[1], seen[2], seen[3], seen[4]
    uv[far] += 1 << 20                                                     # the cell beyond the atlas
    uv[before] -= uv[before, 0] + 5                                        # x0, y0 < 0
    uv[small, 1, 0] = uv[small, 0, 0] + 1                                  # c = 3
    uv[big, 1, 0] = np.iinfo(np.int32).max                                 # c beyond every atlas
    H, W = tex["atlas"].shape[:2]
    uv[edge] += np.array([W, H]) - (uv[edge, 0] - 1) - tex["cell"][edge, 2] + np.array([1, 0])   # one texel over the right edge
    want = P.shade(v, f, uv, tex["atlas"], cams, face)
    out = photo_eval.shade_views(_mesh(v, f), _tex(uv, tex["atlas"]), torch.from_numpy(cams), R.H, R.W)
    _same_image(out["image"].cpu().numpy(), want, "fall-back")
    for k in (far, before, small, big, edge):
        assert not want[0][face[0] == k].any() and plain[0][face[0] == k].any(), k
    assert want.any()
    # no atlas, and no faces: zeros
    out = photo_eval.shade_views(_mesh(v, f), _tex(uv, np.zeros((0, 0, 3), np.uint8)), torch.from_numpy(cams), R.H, R.W)
    assert int(out["image"].sum()) == 0 and int((out["face"] >= 0).sum()) > 0
    out = photo_eval.shade_views(_mesh(v, f[:0]), _tex(uv[:0], tex["atlas"]), torch.from_numpy(cams), R.H, R.W)
    assert int(out["image"].sum()) == 0 and int((out["face"] >= 0).sum()) == 0


def test_shade_a_model_read_back_from_its_obj(tmp_path):
    v, c, f, images, cams, face = P.shade_case("sphere", 3)
    tex, want, _ = P.shade_reference("sphere", 3)
    prefix = str(tmp_path / "model")
    texture.write_textured_obj(prefix, {"vertices": v, "faces": f}, tex)
    got = texture.read_textured_obj(prefix + ".obj")
    H, W = got["atlas"].shape[:2]
    vt = got["vt"][got["face_vt"]]                                        # [NF,3,2]
    uv = np.stack([vt[..., 0] * W, (1.0 - vt[..., 1]) * H], 2)
    assert np.array_equal(uv, np.round(uv)) and np.array_equal(uv.astype(np.int32), tex["uv"])
    out = photo_eval.shade_views(_mesh(got["vertices"], got["faces"]), _tex(uv.astype(np.int32), got["atlas"]), torch.from_numpy(cams),
                                 R.H, R.W)
    _same_image(out["image"].cpu().numpy(), want, "read back")


def test_shade_refuses_cpu_tensors_and_bad_layouts():
    v, c, f, images, cams, face = P.shade_case("sphere", 1)
    tex, _, _ = P.shade_reference("sphere", 1)
    m, t, cam = _mesh(v, f), _tex(tex["uv"], tex["atlas"]), torch.from_numpy(cams)
    for key in ("vertices", "faces"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            photo_eval.shade_views(dict(m, **{key: m[key].cpu()}), t, cam, R.H, R.W)
    for key in ("uv", "atlas"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            photo_eval.shade_views(m, dict(t, **{key: t[key].cpu()}), cam, R.H, R.W)
    for bad in (dict(uv=t["uv"][:-1]), dict(uv=t["uv"].long()), dict(atlas=t["atlas"].float()), dict(atlas=t["atlas"][:, :24])):
        with pytest.raises(ValueError):
            photo_eval.shade_views(m, dict(t, **bad), cam, R.H, R.W)
    with pytest.raises(ValueError, match="chunk"):
        photo_eval.shade_views(m, t, cam, R.H, R.W, chunk=0)


# ------------------------------------------------------------------------------------------------------------------- compare
def _gpu_scores(a, b, mask, **kw):
    out = photo_eval.image_scores(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(mask).cuda(), **kw)
    assert all(t.is_cuda for t in out.values())
    return {k: t.cpu().numpy() for k, t in out.items()}


def _same_bits(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}, expected {want.shape}"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in other places"
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~nan
    assert not bad.any(), f"{what}: differs in {int(bad.sum())} of {bad.size} places, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[bad][0]!r} against {want[bad][0]!r}"


def _compare(a, b, mask, what):
    want = P.scores(a, b, mask)
    got, again = _gpu_scores(a, b, mask, ssim_map=True), _gpu_scores(a, b, mask)
    for k in ("n_px", "sse", "n_win"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), f"{what}: {k} {got[k].tolist()} against {want[k].tolist()}"
    _same_bits(got["ssim_map"], want["ssim_map"], f"{what}: ssim_map")
    bound = want["n_win"][:, None] * 2.0 ** -52 * want["ssim_abs"]         # a sum of n_win terms in any order
    err = np.abs(got["ssim_sum"] - want["ssim_sum"])
    print(f"{what}: n_px {want['n_px'].tolist()}, n_win {want['n_win'].tolist()}, ssim_sum off by at most "
          f"{float((err / np.maximum(bound, 1e-300)).max()):.3g} of the bound, psnr {want['psnr'].tolist()}, ssim {want['ssim'].tolist()}")
    assert (err <= bound).all(), f"{what}: ssim_sum {got['ssim_sum'].tolist()} against {want['ssim_sum'].tolist()}, bound {bound.tolist()}"
    assert np.array_equal(got["ssim_sum"].view(np.uint64), again["ssim_sum"].view(np.uint64)), f"{what}: ssim_sum differs between two runs"
    assert "ssim_map" not in again
    # the host's part: the same formulas on sums that agree to a few ulp
    for k in ("psnr", "ssim", "coverage"):
        assert np.allclose(got[k], want[k], rtol=1e-12, atol=0.0, equal_nan=True), f"{what}: {k} {got[k].tolist()} against {want[k].tolist()}"
    return got, want


@pytest.mark.parametrize("w, h", list(zip(EDGES, EDGES[3:] + EDGES[:3])))
def test_scores_equal_the_restatement_at_every_edge_of_the_tiling(w, h):
    a, b, mask = P.image_pair(1, h, w, seed=w)
    got, want = _compare(a, b, mask, f"{w} x {h}")
    if w < 11 or h < 11:
        assert want["n_win"][0] == 0 and got["ssim_map"].shape == (1, 3, 0, 0) and math.isnan(got["ssim"][0]) and want["n_px"][0] > 0


@pytest.mark.parametrize("w, h", [(TILE + 10, TILE + 10), (2 * TILE + 10, TILE + 11), (11, 11), (12, 2 * TILE + 10)])
def test_scores_with_the_same_edge_on_both_sides(w, h):
    a, b, mask = P.image_pair(1, h, w, seed=3)
    _compare(a, b, mask, f"{w} x {h}")


def test_scores_three_views_in_one_launch_and_a_hole_in_the_mask():
    a, b, mask = P.image_pair(3, 2 * TILE + 5, 3 * TILE + 1, seed=1)
    mask[1, 5:9, 20:30] = 0
    mask[2] = 0
    mask[2, 3:20, 4:30] = 1                                                # a window counts only inside the block
    got, want = _compare(a, b, mask, "three views")
    total = (2 * TILE + 5 - 10) * (3 * TILE + 1 - 10)
    assert all(0 < n < total for n in want["n_win"].tolist()) and len(set(want["n_win"].tolist())) == 3
    assert (np.isnan(want["ssim_map"]).sum((1, 2, 3)) == 3 * (total - want["n_win"])).all()


def test_scores_more_views_than_one_launch_takes():
    a, b, mask = P.image_pair(photo_eval.MAX_CHUNK + 2, 12, 13, seed=2)
    mask[-1, 0, 0] = 0
    _compare(a, b, mask, "34 views")


def test_scores_all_zero_mask():
    a, b, mask = P.image_pair(2, 20, 30)
    got, want = _compare(a, b, np.zeros_like(mask), "empty mask")
    assert (got["n_px"] == 0).all() and (got["n_win"] == 0).all() and (got["sse"] == 0).all() and (got["ssim_sum"] == 0).all()
    assert np.isnan(got["psnr"]).all() and np.isnan(got["ssim"]).all() and (got["coverage"] == 0).all()
    assert np.isnan(got["ssim_map"]).all() and got["ssim_map"].shape == (2, 3, 10, 20)


def test_scores_of_identical_images():
    a = T.view_images(2, TILE + 15, 2 * TILE + 3)
    mask = np.ones(a.shape[:3], np.uint8)
    got, want = _compare(a, a, mask, "a == b")
    assert (got["ssim_map"] == 1.0).all() and (got["ssim"] == 1.0).all() and np.isinf(got["psnr"]).all() and (got["psnr"] > 0).all()
    assert (got["coverage"] == 1.0).all() and (got["n_win"] == (TILE + 5) * (2 * TILE - 7)).all()


def test_scores_take_a_bool_mask_and_refuse_cpu_tensors():
    a, b, mask = P.image_pair(1, 20, 30)
    ta, tb, tm = (torch.from_numpy(x).cuda() for x in (a, b, mask))
    want = photo_eval.image_scores(ta, tb, tm)
    got = photo_eval.image_scores(ta, tb, tm != 0)
    assert all(torch.equal(got[k], want[k]) for k in ("n_px", "sse", "n_win", "ssim_sum"))
    for bad in ((ta.cpu(), tb, tm), (ta, tb.cpu(), tm), (ta, tb, tm.cpu())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            photo_eval.image_scores(*bad)
    for bad in ((ta.float(), tb, tm), (ta, tb[:, :-1], tm), (ta, tb, tm[:, :-1]), (ta, tb, tm.float()), (ta[..., :2], tb[..., :2], tm)):
        with pytest.raises(ValueError):
            photo_eval.image_scores(*bad)
    none = photo_eval.image_scores(ta[:0], tb[:0], tm[:0], ssim_map=True)
    assert none["psnr"].shape == (0,) and none["sse"].shape == (0, 3) and none["ssim_map"].shape == (0, 3, 10, 20)


# -------------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_refuse_what_the_wrappers_never_send():
    lib, E = photo_eval._lib.load(), photo_eval._lib.EINVAL
    t = torch.zeros(4096, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    shade = lambda **k: lib.cds_photo_shade(k.get("vertices", p), k.get("nv", 4), k.get("faces", p), k.get("nf", 4), k.get("uv", p),
                                            k.get("atlas", p), k.get("ah", 4), k.get("aw", 4), k.get("cams", p), k.get("n_views", 1),
                                            k.get("face", p), k.get("h", 4), k.get("w", 4), k.get("image", p), None)
    for bad in (dict(vertices=None), dict(faces=None), dict(uv=None), dict(atlas=None), dict(cams=None), dict(face=None), dict(image=None),
                dict(nv=-1), dict(nv=2 ** 31), dict(nf=-1), dict(nf=2 ** 31), dict(n_views=0), dict(n_views=33), dict(h=0), dict(w=0),
                dict(h=1 << 16, w=1 << 15), dict(aw=12, ah=12), dict(aw=2, ah=2), dict(ah=1), dict(ah=8), dict(aw=0), dict(ah=0),
                dict(aw=1 << 16, ah=1 << 16), dict(aw=-4, ah=-4)):
        assert shade(**bad) == E, bad
    g = (photo_eval.ctypes.c_double * 11)(*photo_eval.gauss_table())
    words = 8                                                              # one view of one tile
    score = lambda **k: lib.cds_photo_scores(k.get("a", p), k.get("b", p), k.get("mask", p), k.get("g", g), k.get("n_views", 1),
                                             k.get("h", 4), k.get("w", 4), k.get("ws", p), k.get("ws_words", words), k.get("counts", p),
                                             k.get("sums", p), None, None)
    for bad in (dict(a=None), dict(b=None), dict(mask=None), dict(g=None), dict(ws=None), dict(counts=None), dict(sums=None),
                dict(n_views=0), dict(n_views=33), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 15), dict(ws_words=words - 1),
                dict(h=17), dict(n_views=2), dict(ws_words=-1)):
        assert score(**bad) == E, bad
    torch.cuda.synchronize()
    assert int(t.abs().sum()) == 0                                         # nothing was written


# ------------------------------------------------------------------------------------------------------------ end to end
FUSE = ["--filter_method", "dynamic", "--conf", "0.0,0.0,0.0", "--dyn_dist_base", "2.0", "--dyn_rel_base", "0.02", "--dyn_views", "1,10"]


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, n), root) for d, _, names in os.walk(root) for n in names)


def _equal(a, b):
    """Two results of score_scan, one of them through JSON: NaN equals NaN."""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_infer_photo_eval_and_the_command_line(tmp_path, capsys):
    """infer --fuse --mesh_voxel --photo_eval on a scene of test_mvs_io._write_scene (4 views of 128 x 160, an untrained network,
    loose consistency settings, as in test_texture_gpu), then python -m cds_mvsnet_amd.photo_eval on the saved output."""
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanA", 4, 128, 160, seed=3)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("scanA\n")
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    base = ["--testpath", root, "--testlist", lst, "--num_view", "3", "--max_h", "128", "--max_w", "160", "--interval_scale", "1.0",
            "--fuse", "--mesh_voxel", "10"] + FUSE
    infer.main(base + ["--outdir", plain])
    capsys.readouterr()
    infer.main(base + ["--outdir", out, "--photo_eval", "--photo_holdout", "2", "--texture_max_cell", "32"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("scanA: psnr ")]
    assert len(lines) == 1 and "held-out" in lines[0] and "over 2 views" in lines[0], lines
    # the score writes no file, and without the options every file is what it was, byte for byte
    before, after = _tree(plain), _tree(out)
    assert before == after and "scanA_mesh.ply" in before
    for name in before:
        assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    # the library call on the saved output gives the line again, and the numbers the command line writes
    want = photo_eval.score_scan(os.path.join(out, "scanA"), os.path.join(out, "scanA_mesh.ply"), os.path.join(root, "scanA"),
                                 holdout=2, max_cell=32)
    assert capsys.readouterr().out.splitlines() == lines
    assert want["views"] == [0, 2] and want["scored"] == 2 and want["textured_from"] == 2 and want["mean"]["coverage"] > 0
    assert all(0.0 < c <= 1.0 for c in want["coverage"]) and all(p > 0 for p in want["psnr"]) and all(-1 <= s <= 1 for s in want["ssim"])
    path = str(tmp_path / "scores.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "cds_mvsnet_amd.photo_eval", "--testpath", root, "--outdir", out, "--testlist", lst,
                          "--holdout", "2", "--texture_max_cell", "32", "--save_renders", "--json", path], env=env, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.splitlines()[0] == lines[0] and res.stdout.splitlines()[1].startswith("mean over 1 scans: psnr ")
    with open(path) as f:
        saved = json.load(f)
    assert _equal(saved["scans"]["scanA"], json.loads(json.dumps(want))) and _equal(saved["mean"], want["mean"])
    assert saved["settings"]["holdout"] == 2 and saved["settings"]["texture"]["max_cell"] == 32
    assert sorted(os.listdir(os.path.join(out, "scanA", "render_photo"))) == ["00000000.png", "00000002.png"]
    # the other modes on the same output: all views, vertex colours, back-facing hits kept
    every = photo_eval.score_scan(os.path.join(out, "scanA"), os.path.join(out, "scanA_mesh.ply"), os.path.join(root, "scanA"), max_cell=32)
    vertex = photo_eval.score_scan(os.path.join(out, "scanA"), os.path.join(out, "scanA_mesh.ply"), os.path.join(root, "scanA"),
                                   holdout=2, colors="vertex", back="keep")
    text = capsys.readouterr().out
    assert every["views"] == [0, 1, 2, 3] and "consistency score" in text and "not a held-out score" in text
    assert vertex["views"] == [0, 2] and all(k >= m for k, m in zip(vertex["coverage"], want["coverage"]))
    with pytest.raises(ValueError, match="holdout"):
        photo_eval.score_scan(os.path.join(out, "scanA"), os.path.join(out, "scanA_mesh.ply"), os.path.join(root, "scanA"), holdout=1)


def test_infer_refuses_photo_options_that_have_nothing_to_work_on(capsys):
    base = ["--testpath", "x", "--testlist", "y", "--outdir", "z"]
    for extra, word in ((["--photo_eval"], "--mesh_voxel"), (["--fuse", "--mesh_voxel", "10", "--photo_holdout", "2"], "--photo_eval"),
                        (["--fuse", "--mesh_voxel", "10", "--photo_eval", "--photo_holdout", "1"], ">= 2")):
        with pytest.raises(SystemExit):
            infer.main(base + extra)
        assert word in capsys.readouterr().err
