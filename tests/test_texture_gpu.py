"""The texturing kernels of csrc/mesh_texture.hip against the numpy restatement of their rule (texture_ref.py):
atlas, uv, view and cell equal in every entry; and the way from a scan's mesh to an OBJ on disk through the command line and
infer --fuse --mesh_voxel --texture."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as R
import texture_ref as T
from cds_mvsnet_amd import infer, mesh, texture
from test_mvs_io import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atlas", "uv", "view", "cell")


def _gpu(v, c, f, images, cams, **kw):
    m = {"vertices": torch.from_numpy(v).cuda(), "colors": torch.from_numpy(c).cuda(), "faces": torch.from_numpy(f).cuda()}
    if isinstance(images, list):
        out, info = texture.texture_mesh(m, [torch.from_numpy(i).cuda() for i in images], [torch.from_numpy(k) for k in cams], **kw)
    else:
        out, info = texture.texture_mesh(m, torch.from_numpy(images).cuda(), torch.from_numpy(cams), **kw)
    assert all(t.is_cuda for t in out.values()) and sorted(out) == sorted(NAMES)
    got = {k: t.cpu().numpy() for k, t in out.items()}
    assert (info["H"], info["W"]) == got["atlas"].shape[:2] and info["unseen"] == int((got["view"] < 0).sum())
    return got


def _same(got, want, what):
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, \
            f"{what}: {k} is {got[k].dtype} {got[k].shape}, expected {want[k].dtype} {want[k].shape}"
        bad = got[k] != want[k]
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} places, first at {np.argwhere(bad)[0].tolist()}"


def _case(name, n_views=1, h=R.H, w=R.W, scale=1.0, max_cell=256, min_px=1, **kw):
    want = T.reference(name, n_views, h, w, scale, max_cell, min_px)
    got = _gpu(*T.case(name, n_views, h, w), scale=scale, max_cell=max_cell, min_px=min_px, **kw)
    sizes = dict(zip(*np.unique(want["cell"][:, 2], return_counts=True)))
    print(f"{name}, {n_views} views of {h} x {w}, scale {scale}, max_cell {max_cell}, min_px {min_px}, {kw}: atlas "
          f"{want['atlas'].shape[1]} x {want['atlas'].shape[0]}, {int((want['view'] >= 0).sum())} of {len(want['view'])} faces seen, cells {sizes}")
    _same(got, want, f"{name} {n_views} {scale} {kw}")
    return got, want


# --------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["plane", "sphere", "clutter", "wild"])
@pytest.mark.parametrize("n_views", [1, 3, 9])
def test_kernels_equal_the_restatement(name, n_views):
    """One view, one chunk of 8 not full, a full chunk plus one view."""
    got, want = _case(name, n_views)
    assert (want["view"] >= 0).any()


def test_chunk_does_not_change_the_result():
    a, _ = _case("sphere", 9, chunk=8)
    for chunk in (1, 4, 32):
        b, _ = _case("sphere", 9, chunk=chunk)
        _same(b, a, f"chunk {chunk}")


def test_both_forms_of_votes_and_fill_give_the_same(monkeypatch):
    a, _ = _case("sphere", 3, scale=8.0, max_cell=16)
    monkeypatch.setattr(texture, "VOTE_RUNS", 1 - texture.VOTE_RUNS)
    monkeypatch.setattr(texture, "FILL_PER_UNIT", 1 - texture.FILL_PER_UNIT)
    b, _ = _case("sphere", 3, scale=8.0, max_cell=16)
    _same(b, a, "other forms")
    _case("clutter", 1, max_cell=64)


def test_of_two_identical_cameras_the_lower_view_wins():
    v, c, f, images, _ = T.case("sphere", 2)
    cams = R.view_cameras(1).repeat(2, 0)
    want = T.texture(v, c, f, images, cams)
    got = _gpu(v, c, f, images, cams)
    _same(got, want, "identical cameras")
    assert set(np.unique(got["view"]).tolist()) == {-1, 0}


@pytest.mark.parametrize("scale", [0.25, 1.0, 8.0])
def test_scale_and_the_clamp_at_max_cell(scale):
    got, want = _case("sphere", 3, scale=scale, max_cell=16)
    sizes = set(np.unique(want["cell"][:, 2]).tolist())
    assert sizes == ({4} if scale == 0.25 else {4, 8} if scale == 1.0 else {4, 16}), sizes     # at 8 every seen face is clamped


def test_clutter_holds_the_largest_and_the_smallest_class():
    got, want = _case("clutter", 1, max_cell=64)
    assert got["cell"][0, 2] == 64 and (got["cell"][2:, 2] == 4).all() and got["view"][1] == -1


def test_plane_that_looks_away_keeps_its_vertex_colours():
    got, want = _case("unseen", 3)
    assert (got["view"] == -1).all() and (got["cell"][:, 2] == 4).all()
    v, c, f, _, _ = T.case("unseen", 3)
    # texel (1, 1) of a cell is corner a moved half a texel: wb = wc = 0.25 for c = 4
    k = 5
    x0, y0 = got["cell"][k, :2]
    col = c[f[k]].astype(np.float64)
    assert np.array_equal(got["atlas"][y0 + 1, x0 + 1], np.floor((0.5 * col[0] + 0.25 * col[1]) + 0.25 * col[2] + 0.5).astype(np.uint8))


def test_min_px_above_every_count():
    got, want = _case("sphere", 3, min_px=10 ** 6)
    assert (got["view"] == -1).all()
    _, some = _case("sphere", 3, min_px=3)
    assert 0 < (some["view"] >= 0).sum() < (T.reference("sphere", 3)["view"] >= 0).sum()


def test_edge_clamp_and_texels_behind_the_camera():
    got, want = _case("special", 1, max_cell=64)
    v, c, f, images, cams = T.case("special", 1)
    assert want["view"].tolist() == [0, 0]
    face, i, j, P = T.texel_points(v, f, want["cell"][:, 2])
    u, vv, z = T._project(cams[0], P)
    corner, slanted = face == 0, face == 1
    print(f"corner face: {int((corner & (u < 0.5) & (vv < 0.5)).sum())} texels clamped at both edges; slanted face: "
          f"{int((slanted & ~(z > 0)).sum())} of {int(slanted.sum())} texels behind the camera")
    assert (corner & (u < 0) & (vv < 0)).any() and (slanted & ~(z > 0)).any() and (slanted & (z > 0)).any()


def test_image_one_pixel_wide():
    got, want = _case("special", 1, R.H, 1)
    assert want["view"][0] == 0


def test_map_of_50_by_37():
    _case("wild", 2, 37, 50)
    _case("sphere", 2, 37, 50)


def test_views_of_two_image_sizes():
    """Three views of 64 x 48 and two of 50 x 37 in one atlas: the views are numbered through the groups, faces take their colour
    from both, and one group given as a list equals the plain call."""
    v, c, f, images, _ = T.case("sphere", 3)
    cams, small = R.view_cameras(5), T.view_images(2, 37, 50, seed=5)
    want = T.texture(v, c, f, [images, small], [cams[:3], cams[3:]])
    for chunk in (8, 2):
        _same(_gpu(v, c, f, [images, small], [cams[:3], cams[3:]], chunk=chunk), want, f"two sizes, chunk {chunk}")
    assert set(np.unique(want["view"]).tolist()) == {-1, 0, 1, 2, 3, 4}
    _same(_gpu(v, c, f, [images], [cams[:3]]), T.reference("sphere", 3), "one group as a list")
    # the small views first: other numbers, the same rule
    _same(_gpu(v, c, f, [small, images], [cams[3:], cams[:3]]), T.texture(v, c, f, [small, images], [cams[3:], cams[:3]]), "small first")
    m = {"vertices": torch.from_numpy(v).cuda(), "colors": torch.from_numpy(c).cuda(), "faces": torch.from_numpy(f).cuda()}
    with pytest.raises(ValueError, match="lists"):
        texture.texture_mesh(m, [torch.from_numpy(images).cuda()], torch.from_numpy(cams[:3]))
    with pytest.raises(ValueError, match="lists"):
        texture.texture_mesh(m, [torch.from_numpy(images).cuda()], [])


# ---------------------------------------------------------------------------------------------------------------- errors
def test_empty_mesh_zero_views_and_cpu_tensors(monkeypatch):
    v, c, f, images, cams = T.case("plane", 2)
    m = {"vertices": torch.from_numpy(v).cuda(), "colors": torch.from_numpy(c).cuda(), "faces": torch.from_numpy(f).cuda()}
    ti, tc = torch.from_numpy(images).cuda(), torch.from_numpy(cams)

    def no_launch():
        raise AssertionError("the library was loaded: a launch was about to happen")
    monkeypatch.setattr(texture._lib, "load", no_launch)
    monkeypatch.setattr(texture, "render_mesh", lambda *a, **k: no_launch())
    out, info = texture.texture_mesh(dict(m, faces=m["faces"][:0]), ti, tc)
    assert out["atlas"].shape == (0, 0, 3) and out["uv"].shape == (0, 3, 2) and out["view"].shape == (0,) and info["H"] == 0
    out, info = texture.texture_mesh(m, ti[:0], tc[:0])
    assert out["atlas"].shape == (0, 0, 3) and out["uv"].shape == (len(f), 3, 2) and int((out["view"] != -1).sum()) == 0
    assert out["cell"].dtype == torch.int32 and int(out["cell"].abs().sum()) == 0 and info["unseen"] == len(f)
    for bad in (dict(images=ti.float()), dict(cams=tc[:1]), dict(scale=0.0), dict(max_cell=24), dict(chunk=0)):
        kw = dict(images=ti, cams=tc)
        kw.update(bad)
        with pytest.raises(ValueError):
            texture.texture_mesh(m, **kw)
    g = m["faces"].clone()
    g[3, 1] = len(v)
    with pytest.raises(ValueError, match="outside"):
        texture.texture_mesh(dict(m, faces=g), ti, tc)
    for key in ("vertices", "colors", "faces"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            texture.texture_mesh(dict(m, **{key: m[key].cpu()}), ti, tc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        texture.texture_mesh(m, ti.cpu(), tc)


def test_atlas_wider_than_max_size_is_refused():
    v, c, f, images, cams = T.case("sphere", 1)
    m = {"vertices": torch.from_numpy(v).cuda(), "colors": torch.from_numpy(c).cuda(), "faces": torch.from_numpy(f).cuda()}
    with pytest.raises(ValueError, match="--texture_scale"):
        texture.texture_mesh(m, torch.from_numpy(images).cuda(), torch.from_numpy(cams), max_size=64)


def test_entry_points_refuse_what_the_wrapper_never_sends():
    lib, E = texture._lib.load(), texture._lib.EINVAL
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    assert lib.cds_texture_votes(p, p, 0, 4, 4, 4, p, 1, None) == E and lib.cds_texture_votes(p, p, 33, 4, 4, 4, p, 1, None) == E
    assert lib.cds_texture_votes(p, p, 1, 4, 4, 4, p, 2, None) == E and lib.cds_texture_votes(p, None, 1, 4, 4, 4, p, 1, None) == E
    assert lib.cds_texture_best(p, 4, 0, 0, p, None) == E and lib.cds_texture_best(p, 4, 1, -1, p, None) == E
    assert lib.cds_texture_cells(p, 4, p, 4, p, 1, p, 0, 1.0, 16, p, p, None) == E
    assert lib.cds_texture_cells(p, 4, p, 4, p, 1, p, 1, 0.0, 16, p, p, None) == E
    assert lib.cds_texture_cells(p, 4, p, 4, p, 1, p, 1, 1.0, 24, p, p, None) == E
    assert lib.cds_texture_place(p, p, 4, -1, 16, p, p, None) == E and lib.cds_texture_place(p, p, 4, 4, 3, p, p, None) == E
    fill = lambda **k: lib.cds_texture_fill(p, p, 4, p, 4, p, p, k.get("image_bytes", 48), k.get("views", p), k.get("n_views", 1), p, p,
                                            p, p, k.get("total", 1), 16, k.get("ah", 4), k.get("aw", 4), k.get("atlas", p),
                                            k.get("per_unit", 0), None)
    for bad in (dict(image_bytes=-1), dict(views=None), dict(n_views=0), dict(total=2), dict(aw=12, ah=12), dict(ah=1), dict(atlas=None), dict(atlas=p + 1), dict(per_unit=2), dict(total=-1)):
        assert fill(**bad) == E, bad
    torch.cuda.synchronize()
    assert int(t.abs().sum()) == 0                                   # nothing was written


# ------------------------------------------------------------------------------------------------------------ end to end
FUSE = ["--filter_method", "dynamic", "--conf", "0.0,0.0,0.0", "--dyn_dist_base", "2.0", "--dyn_rel_base", "0.02", "--dyn_views", "1,10"]


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, n), root) for d, _, names in os.walk(root) for n in names)


def test_infer_texture_and_the_command_line(tmp_path, capsys):
    """infer --fuse --mesh_voxel --texture on a scene of test_mvs_io._write_scene (3 views of 128 x 160, an untrained network, loose
    consistency settings, as in test_render_gpu), then python -m cds_mvsnet_amd.texture on the saved output."""
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanA", 3, 128, 160, seed=3)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("scanA\n")
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    base = ["--testpath", root, "--testlist", lst, "--num_view", "3", "--max_h", "128", "--max_w", "160", "--interval_scale", "1.0",
            "--fuse", "--mesh_voxel", "10"] + FUSE
    infer.main(base + ["--outdir", plain])
    infer.main(base + ["--outdir", out, "--texture", "--texture_max_cell", "32"])
    assert [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("scanA_textured.obj: atlas ")]
    # without --texture: no textured files, and every other file is the same, byte for byte
    new = [f"scanA_textured.{e}" for e in ("mtl", "obj", "png")]
    before, after = _tree(plain), _tree(out)
    assert sorted(before + new) == after and "scanA_mesh.ply" in before
    for name in before:
        assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    # the OBJ reads back to the mesh written, every vt inside its face's cell, and the files are texture_mesh of the saved inputs
    v, c, f = mesh.read_mesh_ply(os.path.join(out, "scanA_mesh.ply"))
    assert len(f) > 0
    got = texture.read_textured_obj(os.path.join(out, "scanA_textured.obj"))
    assert np.array_equal(got["vertices"].view(np.uint32), v.view(np.uint32)) and np.array_equal(got["faces"], f)
    from PIL import Image
    from cds_mvsnet_amd import mvs_io
    cams, images = [], []
    for i in range(3):
        intr, extr, _, _ = mvs_io.read_cam_file(os.path.join(out, "scanA", "cams", f"{i:08d}_cam.txt"))
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3] = extr, intr
        cams.append(cam)
        images.append(np.asarray(Image.open(os.path.join(out, "scanA", "images", f"{i:08d}.jpg")).convert("RGB")))
    again = _gpu(v, c, f, np.stack(images), np.stack(cams), max_cell=32)
    H, W = again["atlas"].shape[:2]
    print(f"{len(f)} faces: atlas {W} x {H}, {int((again['view'] >= 0).sum())} seen")
    assert np.array_equal(got["atlas"], again["atlas"]) and (again["view"] >= 0).any()
    x, y = got["vt"][:, 0].reshape(-1, 3) * W, (1.0 - got["vt"][:, 1].reshape(-1, 3)) * H
    assert np.array_equal(np.stack([x, y], 2), again["uv"].astype(np.float64))
    cell = again["cell"]
    assert ((x > cell[:, :1]) & (x < cell[:, :1] + cell[:, 2:]) & (y > cell[:, 1:2]) & (y < cell[:, 1:2] + cell[:, 2:])).all()
    # ... and equal to the restatement of the rule
    _same(again, T.texture(v, c, f, np.stack(images), np.stack(cams), max_cell=32), "scene mesh")
    # the command line on the saved output reproduces the three files
    saved = {n: open(os.path.join(out, n), "rb").read() for n in new}
    for n in new:
        os.remove(os.path.join(out, n))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "cds_mvsnet_amd.texture", "--testpath", root, "--outdir", out, "--testlist", lst,
                          "--texture_max_cell", "32"], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "scanA_textured.obj: atlas " in res.stdout
    assert {n: open(os.path.join(out, n), "rb").read() for n in new} == saved
    # a scan whose saved images differ in size: the views grouped by size as render_scan groups its maps, numbered through the groups
    small = os.path.join(out, "scanA", "images", "00000001.jpg")
    Image.fromarray(np.ascontiguousarray(images[1][::2, ::2])).save(small, quality=95)
    info = texture.texture_scan(os.path.join(out, "scanA"), os.path.join(out, "scanA_mesh.ply"), os.path.join(root, "scanA"),
                                str(tmp_path / "mixed"), max_cell=32)
    half = np.array(Image.open(small).convert("RGB"))
    mixed = _gpu(v, c, f, [np.stack([images[0], images[2]]), half[None]], [np.stack([cams[0], cams[2]]), cams[1][None]], max_cell=32)
    assert info["views"] == 3 and half.shape == (64, 80, 3) and info["unseen"] == int((mixed["view"] < 0).sum())
    assert np.array_equal(texture.read_textured_obj(str(tmp_path / "mixed.obj"))["atlas"], mixed["atlas"])
