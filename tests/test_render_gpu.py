"""The rasteriser kernels of csrc/raster.hip against the numpy restatement of their rule (render_ref.py): every
output bit for bit; and the way from a scan's mesh to depth maps on disk and a tree to train from, through render_scan, the
command line and infer --fuse --mesh_voxel --render_mesh."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_ref as M
import render_ref as R
from cds_mvsnet_amd import _lib, infer, mesh, mvs_io, render
from test_mvs_io import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("depth", "face", "front", "valid", "image")


def _gpu(v, f, cams, h, w, c=None, **kw):
    out = render.render_mesh(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(cams), h, w,
                             colors=None if c is None else torch.from_numpy(c).cuda(), **kw)
    assert all(t.is_cuda for t in out.values())
    return {k: t.cpu().numpy() for k, t in out.items()}


def _same(got, want, what):
    """Every output equal; depth by its bits."""
    assert sorted(got) == sorted(want), what
    for k in NAMES:
        if k not in want:
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what}: {k} is {got[k].dtype} {got[k].shape}"
        a, b = (got[k].view(np.uint32), want[k].view(np.uint32)) if k == "depth" else (got[k], want[k])
        bad = a != b
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} places, first at {np.argwhere(bad)[0].tolist()}"


def _case(name, n_views=1, h=R.H, w=R.W, **kw):
    v, f, c, cams, want = R.reference(name, n_views, h, w)
    got = _gpu(v, f, cams, h, w, c, **kw)
    hit = want["face"] >= 0
    print(f"{name}, {n_views} views of {h} x {w}, {kw}: {int(hit.sum())} hits, {len(np.unique(want['face'][hit]))} faces seen, "
          f"{int((want['front'][hit] == 0).sum())} back-facing")
    assert hit.any()
    _same(got, want, f"{name} {n_views} {kw}")
    return got


# --------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["plane", "sphere"])
@pytest.mark.parametrize("n_views", [1, 3, 9])
def test_plane_and_sphere_vs_restatement(name, n_views):
    """One view, one chunk of 8 not full, a full chunk plus one view."""
    _case(name, n_views)


@pytest.mark.parametrize("name,n_views", [("plane", 2), ("sphere", 3), ("clutter", 1), ("wild", 9)])
def test_large_px_does_not_change_the_result(name, n_views):
    """large_px 1: every face with more than one candidate on the wave path; 64: mixed; 10^9: everything per thread."""
    outs = [_case(name, n_views, large_px=lp) for lp in (1, 64, 10 ** 9)]
    for o in outs[1:]:
        _same(o, outs[0], name)


def test_two_map_spanning_faces_and_sub_pixel_faces():
    """Two triangles that cover the 64 x 48 map (3072 candidates each: the wave path, ceil(h w / 64) iterations per lane) behind
    200 sub-pixel ones, some of which contain a pixel centre."""
    got = _case("clutter")
    assert (got["face"] >= 0).all() and (got["face"] >= 2).sum() >= 20
    assert set(np.unique(got["front"][got["face"] < 2]).tolist()) == {0, 1}       # one of the two looks away


@pytest.mark.parametrize("name", ["plane", "sphere", "wild"])
def test_map_of_50_by_37(name):
    _case(name, 2, 37, 50)


def test_unusable_vertices_drop_their_faces():
    """Vertices behind the camera, at 1e30, infinite and NaN, beyond the 2^28 limit; a usable one far outside the map; a
    degenerate face (test_render_cpu checks that wild_mesh() holds them)."""
    got = _case("wild", 3)
    n_plane = len(R.plane_mesh()[1])
    seen = np.unique(got["face"][0])
    assert n_plane + 7 in seen and not set(seen.tolist()) & {n_plane + k for k in (0, 1, 2, 4, 5, 6, 10)}


def test_depths_that_differ_in_the_last_bit():
    got = _case("last_bit")
    assert np.unique(got["face"]).tolist() == [-1, 0, 3, 4, 7, 8, 11, 12, 15]      # the nearer face of every pair, not the first


def _analytic():
    vol, m = M.analytic_case("sphere")
    spec = M.ANALYTIC["sphere"]
    cams = M.sphere_scene(radius_vox=spec["radius"], voxel=1.0, size=48, centre=spec["centre"])["cams"]
    return m["vertices"], m["faces"], m["colors"], cams


def test_extracted_sphere_from_26_cameras():
    """The mesh of mesh_ref.analytic_case("sphere") (4568 faces in block-key order, the winding of §1.9) from 26 cameras around it
    at 48 x 48: three full chunks and two views.  Its faces look at the camera but for slivers on the silhouette."""
    v, f, c, cams = _analytic()
    want = R.render(v, f, cams, 48, 48, c)
    got = _gpu(v, f, cams, 48, 48, c)
    _same(got, want, "extracted sphere")
    hit = got["face"] >= 0
    print(f"extracted sphere: {hit.mean():.3f} of the pixels hit, {(got['front'][hit] == 1).mean():.5f} of them front-facing")
    assert len(cams) == 26 and hit.mean() > 0.3 and (got["front"][hit] == 1).mean() > 0.999


def test_chunk_and_repetition_do_not_change_the_result():
    v, f, c, cams = _analytic()
    args = (torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(cams), 48, 48, torch.from_numpy(c).cuda())
    a = render.render_mesh(*args, chunk=8)
    for kw in (dict(chunk=1), dict(chunk=8), dict(chunk=32, large_px=3)):
        b = render.render_mesh(*args, **kw)
        for k in NAMES:
            assert torch.equal(a[k], b[k]), (k, kw)
    # without colours: no image, the rest unchanged
    b = render.render_mesh(*args[:5])
    assert "image" not in b and all(torch.equal(a[k], b[k]) for k in NAMES[:4])


# ---------------------------------------------------------------------------------------------------------------- errors
def test_invalid_arguments_raise_before_any_launch(monkeypatch):
    v, f, c, cams, _ = R.reference("plane", 2)
    tv, tf, tc, tcam = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(cams)

    def no_launch():
        raise AssertionError("the library was loaded: a launch was about to happen")
    monkeypatch.setattr(render._lib, "load", no_launch)
    for bad in (dict(vertices=tv[:, :2]), dict(vertices=tv.double()), dict(faces=tf.long()), dict(faces=tf.reshape(-1)),
                dict(colors=tc[:-1]), dict(colors=tc.float()), dict(cams=tcam[:, 0]), dict(h=0), dict(chunk=0), dict(chunk=33),
                dict(large_px=0)):
        kw = dict(vertices=tv, faces=tf, cams=tcam, h=R.H, w=R.W, colors=tc)
        kw.update(bad)
        with pytest.raises(ValueError):
            render.render_mesh(**kw)
    for bad in (dict(vertices=tv.cpu()), dict(faces=tf.cpu()), dict(colors=tc.cpu())):
        kw = dict(vertices=tv, faces=tf, cams=tcam, h=R.H, w=R.W, colors=tc)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            render.render_mesh(**kw)
    for row, col, val in ((2, 2, 2.0), (2, 0, 1e-3), (2, 1, -1.0), (1, 0, 0.25)):
        k = tcam.clone()
        k[1, 1, row, col] = val
        with pytest.raises(ValueError, match="view 1"):
            render.render_mesh(tv, tf, k, R.H, R.W)
    for idx in (-1, len(v)):
        g = tf.clone()
        g[5, 1] = idx
        with pytest.raises(ValueError, match="outside"):
            render.render_mesh(tv, g, tcam, R.H, R.W)
    # an empty mesh and zero views: all-miss or empty outputs, still without a launch
    out = render.render_mesh(tv, tf[:0], tcam, R.H, R.W, colors=tc)
    assert out["depth"].shape == (2, R.H, R.W) and float(out["depth"].abs().sum()) == 0 and int((out["face"] != -1).sum()) == 0
    assert int(out["valid"].sum()) == 0 and int(out["front"].sum()) == 0 and out["image"].shape == (2, R.H, R.W, 3)
    out = render.render_mesh(tv[:0], tf[:0], tcam, R.H, R.W)
    assert int((out["face"] != -1).sum()) == 0 and "image" not in out
    out = render.render_mesh(tv, tf, tcam[:0], R.H, R.W, colors=tc)
    assert out["depth"].shape == (0, R.H, R.W) and out["image"].shape == (0, R.H, R.W, 3) and out["face"].dtype == torch.int32


def test_entry_points_refuse_what_the_wrapper_never_sends():
    lib = _lib.load()
    v, f, c, cams, want = R.reference("plane", 1)
    tv, tf = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    tab = render.camera_table(torch.from_numpy(cams)).cuda()
    nv, nf, h, w = len(v), len(f), R.H, R.W
    xy = torch.empty((1, nv, 2), dtype=torch.int32, device="cuda")
    xc = torch.empty((1, nv, 3), dtype=torch.float64, device="cuda")
    keys = torch.full((1, h, w), -1, dtype=torch.int64, device="cuda")
    large = torch.zeros((1, nf), dtype=torch.uint8, device="cuda")
    E = _lib.EINVAL
    assert lib.cds_raster_project(tv.data_ptr(), nv, tab.data_ptr(), 0, xy.data_ptr(), xc.data_ptr(), None) == E
    assert lib.cds_raster_project(tv.data_ptr(), nv, tab.data_ptr(), 33, xy.data_ptr(), xc.data_ptr(), None) == E
    assert lib.cds_raster_project(tv.data_ptr(), -1, tab.data_ptr(), 1, xy.data_ptr(), xc.data_ptr(), None) == E
    assert lib.cds_raster_project(tv.data_ptr(), nv, None, 1, xy.data_ptr(), xc.data_ptr(), None) == E
    face_args = lambda **k: [k.get("faces", tf.data_ptr()), k.get("nf", nf), nv, tab.data_ptr(), k.get("views", 1), xy.data_ptr(),
                             xc.data_ptr(), k.get("h", h), w, k.get("large_px", 64), keys.data_ptr(), k.get("large", large.data_ptr()), None]
    for bad in (dict(large_px=0), dict(h=0), dict(h=1 << 30), dict(views=0), dict(nf=-1), dict(nf=1 << 31), dict(large=None),
                dict(faces=None)):
        assert lib.cds_raster_faces(*face_args(**bad)) == E, bad
    lst = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert lib.cds_raster_large(lst.data_ptr(), -1, tf.data_ptr(), nf, nv, tab.data_ptr(), 1, xy.data_ptr(), xc.data_ptr(), h, w,
                                keys.data_ptr(), None) == E
    assert lib.cds_raster_large(lst.data_ptr(), (1 << 30) + 1, tf.data_ptr(), nf, nv, tab.data_ptr(), 1, xy.data_ptr(), xc.data_ptr(),
                                h, w, keys.data_ptr(), None) == E
    assert lib.cds_raster_large(None, 4, tf.data_ptr(), nf, nv, tab.data_ptr(), 1, xy.data_ptr(), xc.data_ptr(), h, w,
                                keys.data_ptr(), None) == E
    d = torch.empty((1, h, w), dtype=torch.float32, device="cuda")
    assert lib.cds_raster_resolve(keys.data_ptr(), tf.data_ptr(), nf, nv, tab.data_ptr(), 1, xc.data_ptr(), None, h, w, d.data_ptr(),
                                  None, None, None, None, None) == E
    torch.cuda.synchronize()
    assert int((keys != -1).sum()) == 0                             # nothing was drawn
    # entries of the list that do not belong to the chunk, and a face index outside the vertices, draw nothing and read nothing
    assert lib.cds_raster_project(tv.data_ptr(), nv, tab.data_ptr(), 1, xy.data_ptr(), xc.data_ptr(), None) == 0
    lst = torch.tensor([-1, nf, 1 << 40], dtype=torch.int64, device="cuda")
    assert lib.cds_raster_large(lst.data_ptr(), 3, tf.data_ptr(), nf, nv, tab.data_ptr(), 1, xy.data_ptr(), xc.data_ptr(), h, w,
                                keys.data_ptr(), None) == 0
    wrong = tf.clone()
    wrong[:, 2] = nv
    wrong[::2, 2] = -5
    assert lib.cds_raster_faces(*face_args(faces=wrong.data_ptr())) == 0
    torch.cuda.synchronize()
    assert int((keys != -1).sum()) == 0 and int(large.sum()) == 0
    # the entry points alone, in the wrapper's order, give the restatement
    assert lib.cds_raster_faces(*face_args(large_px=2)) == 0
    todo = torch.nonzero(large.reshape(-1)).reshape(-1)
    assert 0 < todo.numel() <= nf
    assert lib.cds_raster_large(todo.data_ptr(), todo.numel(), tf.data_ptr(), nf, nv, tab.data_ptr(), 1, xy.data_ptr(), xc.data_ptr(),
                                h, w, keys.data_ptr(), None) == 0
    out = {k: torch.empty((1, h, w), dtype=t, device="cuda") for k, t in render.OUTPUTS}
    assert lib.cds_raster_resolve(keys.data_ptr(), tf.data_ptr(), nf, nv, tab.data_ptr(), 1, xc.data_ptr(), None, h, w,
                                  out["depth"].data_ptr(), out["face"].data_ptr(), out["front"].data_ptr(), out["valid"].data_ptr(),
                                  None, None) == 0
    _same({k: t.cpu().numpy() for k, t in out.items()}, {k: want[k] for k in NAMES[:4]}, "entry points")


# ------------------------------------------------------------------------------------------------------------ end to end
FUSE = ["--filter_method", "dynamic", "--conf", "0.0,0.0,0.0", "--dyn_dist_base", "2.0", "--dyn_rel_base", "0.02", "--dyn_views", "1,10"]


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, n), root) for d, _, names in os.walk(root) for n in names)


def _child(module, argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", module] + argv, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout


def test_infer_render_mesh_and_export(tmp_path, capsys):
    """infer --fuse --mesh_voxel --render_mesh --export_blended on a scene of test_mvs_io._write_scene (3 views of 128 x 160, an
    untrained network, loose consistency settings, as in test_mesh_gpu.test_infer_fuse_mesh)."""
    from cds_mvsnet_amd import train_data as TD
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanA", 3, 128, 160, seed=3)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("scanA\n")
    plain, out, D = str(tmp_path / "plain"), str(tmp_path / "out"), str(tmp_path / "blended")
    base = ["--testpath", root, "--testlist", lst, "--num_view", "3", "--max_h", "128", "--max_w", "160", "--interval_scale", "1.0",
            "--fuse", "--mesh_voxel", "10"] + FUSE
    infer.main(base + ["--outdir", plain])
    infer.main(base + ["--outdir", out, "--render_mesh", "--export_blended", D])
    lines = capsys.readouterr().out.splitlines()
    assert [ln for ln in lines if "scanA/depth_mesh:" in ln and "% valid" in ln and "back-facing" in ln]
    # without --render_mesh: no depth_mesh, and every other file is the same, byte for byte
    before, after = _tree(plain), _tree(out)
    new = [f"scanA/depth_mesh/{i:08d}.pfm" for i in range(3)]
    assert not os.path.exists(os.path.join(plain, "scanA", "depth_mesh")) and sorted(before + new) == after
    assert "scanA.ply" in before and "scanA_mesh.ply" in before
    for name in before:
        assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    # the files are render_mesh of the mesh read back, with valid applied
    v, c, f = mesh.read_mesh_ply(os.path.join(out, "scanA_mesh.ply"))
    assert len(f) > 0
    cams = []
    for i in range(3):
        intr, extr, _, _ = mvs_io.read_cam_file(os.path.join(out, "scanA", "cams", f"{i:08d}_cam.txt"))
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3] = extr, intr
        cams.append(cam)
    got = _gpu(v, f, np.stack(cams), 128, 160)
    want = np.where(got["valid"] != 0, got["depth"], np.float32(0))
    maps = np.stack([mvs_io.read_pfm(os.path.join(out, new[i]))[0] for i in range(3)])
    est = np.stack([mvs_io.read_pfm(os.path.join(out, "scanA", "depth_est", f"{i:08d}.pfm"))[0] for i in range(3)])
    print(f"{len(f)} faces: {(got['face'] >= 0).mean():.3f} of the pixels hit, {(want > 0).mean():.3f} valid")
    assert maps.shape == (3, 128, 160) and np.array_equal(maps.view(np.uint32), want.view(np.uint32)) and (want > 0).any()
    # ... and equal to the restatement of the rule
    ref = R.render(v, f, np.stack(cams), 128, 160)
    _same(got, ref, "scene mesh")
    # the command line on the saved output reproduces the files and the exported tree
    saved = {n: open(os.path.join(out, n), "rb").read() for n in new}
    tree = {n: open(os.path.join(D, n), "rb").read() for n in _tree(D)}
    assert sorted(tree) == sorted([f"scanA/{sub}/{i:08d}{ext}" for i in range(3) for sub, ext in
                                   (("blended_images", ".jpg"), ("cams", "_cam.txt"), ("rendered_depth_maps", ".pfm"))] +
                                  ["scanA/cams/pair.txt"])
    for n in new:
        os.remove(os.path.join(out, n))
    D2 = str(tmp_path / "blended2")
    stdout = _child("cds_mvsnet_amd.render", ["--testpath", root, "--outdir", out, "--testlist", lst, "--export_blended", D2])
    assert "scanA/depth_mesh: 3 views" in stdout
    assert {n: open(os.path.join(out, n), "rb").read() for n in new} == saved
    assert {n: open(os.path.join(D2, n), "rb").read() for n in _tree(D2)} == tree
    # the exported tree: the saved images and maps, the scene's pairs and depth range, the cameras of the saved resolution
    for i in range(3):
        assert tree[f"scanA/blended_images/{i:08d}.jpg"] == open(os.path.join(out, "scanA", "images", f"{i:08d}.jpg"), "rb").read()
        assert tree[f"scanA/rendered_depth_maps/{i:08d}.pfm"] == saved[new[i]]
        intr, extr, dmin, dint = mvs_io.read_cam_file(os.path.join(D, "scanA", "cams", f"{i:08d}_cam.txt"))
        assert np.array_equal(intr, cams[i][1, :3, :3]) and np.array_equal(extr, cams[i][0]) and (dmin, dint) == (425.0, 2.5)
    assert tree["scanA/cams/pair.txt"] == open(os.path.join(root, "scanA", "pair.txt"), "rb").read()
    # ... loads as a training set
    ds = TD.BlendedTrainScenes(D, lst, "train", 3, crop=(128, 160))
    with TD.TrainBatches(ds, 1, "cuda", ahead=0) as it:
        batch = next(it)
    assert tuple(batch["imgs"].shape) == (1, 3, 3, 128, 160) and tuple(batch["depth"]["stage3"].shape) == (1, 64, 80)
    assert int((batch["mask"]["stage3"] > 0).sum()) > 0
    # --back keep adds the back-facing hits; --max_rel_diff 0 keeps a pixel only where the bits agree with depth_est (or depth_est has
    # none); a huge value changes nothing
    scan, pairs = os.path.join(out, "scanA"), os.path.join(root, "scanA")
    mesh_file = os.path.join(out, "scanA_mesh.ply")

    def again(sub, **kw):
        render.render_scan(scan, mesh_file, pairs, subdir=sub, **kw)
        return np.stack([mvs_io.read_pfm(os.path.join(scan, sub, f"{i:08d}.pfm"))[0] for i in range(3)])
    keep = again("keep", back="keep")
    assert np.array_equal(keep.view(np.uint32), np.where(got["face"] >= 0, got["depth"], np.float32(0)).view(np.uint32))
    zero = again("r0", max_rel_diff=0.0)
    agree = ~((est > 0) & (est != maps))
    assert np.array_equal(zero.view(np.uint32), np.where(agree, maps, np.float32(0)).view(np.uint32)) and (zero > 0).sum() < (maps > 0).sum()
    assert np.array_equal(again("huge", max_rel_diff=1e30).view(np.uint32), maps.view(np.uint32))
    some = again("r5", max_rel_diff=0.05)
    assert np.array_equal(some > 0, (maps > 0) & ~((est > 0) & (np.abs(maps - est) > np.float32(0.05) * maps)))
    # the colour render
    render.render_scan(scan, mesh_file, pairs, subdir="img", save_image=True)
    assert sorted(os.listdir(os.path.join(scan, "img"))) == sorted([f"{i:08d}{e}" for i in range(3) for e in (".pfm", ".jpg")])
    assert open(os.path.join(scan, "img", "00000001.pfm"), "rb").read() == saved[new[1]]
