"""Fused clouds with normals and voxel merging on the MI355X: cds_depth_normals_f32 and cds_voxel_merge_f32
against the float64 restatements of tests/cloud_ref.py, the tile and halo shapes of the normals kernel, its properties, the
argument checks, and the way through filter_depth, the command line and infer --fuse.

Bounds.  ``ok`` is exact by construction, so no pixel may differ.  A normal is a unit vector rounded once to float32: 6e-8 per
component; 1e-6 leaves room for the float64 differences between the kernel's adjugate form and the restatement's
``np.linalg.solve``.  The merged positions must be the bits of ``tt_eval.voxel_down_sample``; colours and counts are integers."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_ref as C
from cds_mvsnet_amd import _lib, fusion, infer, mvs_io, ops, pointcloud, synth, tt_eval
from test_mvs_io import _write_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"s3x24x40": (3, 24, 40, 0), "s4x48x64": (4, 48, 64, 5)}
NORMAL_TOL = 1e-6
CONF = (0.1, 0.1, 0.1)


@functools.lru_cache(maxsize=None)
def _scene(name):
    n, h, w, seed = SCENES[name]
    return synth.make_fusion_scene(n, h, w, seed=seed, outlier_frac=0.15)


@functools.lru_cache(maxsize=None)
def _scene_reference(name, view):
    sc = _scene(name)
    cam = sc["cams"][view].numpy()
    return C.depth_normals(sc["depths"][view].numpy(), cam[1, :3, :3], cam[0], radius=2, jump=0.01, min_pts=6)


def _kernel(depth, K, E, valid=None, **kw):
    d = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).cuda()
    v = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, dtype=np.uint8)).cuda()
    nrm, ok = ops.depth_normals(d, torch.from_numpy(np.asarray(K, np.float32)), torch.from_numpy(np.asarray(E, np.float32)),
                                valid=v, **kw)
    assert nrm.dtype == torch.float32 and ok.dtype == torch.uint8
    assert tuple(nrm.shape) == (3,) + tuple(d.shape) and tuple(ok.shape) == tuple(d.shape)
    return nrm.cpu().numpy(), ok.cpu().numpy()


def _compare(got, want, what):
    (gn, gok), (wn, wok) = got, want
    diff = int((gok != wok).sum())
    err = float(np.abs(gn.astype(np.float64) - wn)[:, wok > 0].max()) if (wok > 0).any() else 0.0
    print(f"{what}: ok share {wok.mean():.3f}, ok differs in {diff} pixels, normals max-abs {err:.2e}")
    assert set(np.unique(gok).tolist()) <= {0, 1}
    assert diff == 0
    assert err <= NORMAL_TOL
    assert (gn[:, gok == 0] == 0).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_is_well_populated(name):
    shares = [float(_scene_reference(name, v)[1].mean()) for v in range(SCENES[name][0])]
    print(f"{name}: ok share per view {', '.join(f'{s:.3f}' for s in shares)}")
    assert all(0.5 <= s <= 0.95 for s in shares)


@pytest.mark.parametrize("name", list(SCENES))
def test_normals_vs_reference_on_the_scenes(name):
    sc = _scene(name)
    for v in range(SCENES[name][0]):
        cam = sc["cams"][v].numpy()
        got = _kernel(sc["depths"][v].numpy(), cam[1, :3, :3], cam[0], radius=2, jump=0.01, min_pts=6)
        _compare(got, _scene_reference(name, v), f"{name} view {v}")


def _rough_case(h, w, seed):
    """A bumpy tilted plane with 15 % depth outliers, a few 0 / NaN / inf depths, and a valid map with random holes and a
    full zero row and column."""
    rs = np.random.RandomState(seed)
    depth, K, E, _ = C.tilted_plane(h, w, np.float64, f=max(1.2 * w, 60.0))
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    depth = depth * (1.0 + 0.002 * np.sin(xs / 3.0) * np.cos(ys / 2.0))
    bad = rs.rand(h, w) < 0.15
    depth = np.where(bad, depth * (1.0 + rs.choice([-1.0, 1.0], (h, w)) * rs.uniform(0.02, 0.06, (h, w))), depth).astype(np.float32)
    for val in (0.0, np.nan, np.inf, -np.inf, -3.0):
        depth[rs.randint(h), rs.randint(w)] = val
    valid = (rs.rand(h, w) > 0.1).astype(np.uint8)
    valid[h // 2, :] = 0
    valid[:, w // 3] = 0
    return depth, K, E, valid


SHAPES = [(1, 1, 1), (1, 1, 4), (3, 3, 4), (3, 3, 1), (5, 67, 1), (5, 67, 2), (5, 67, 3), (5, 67, 4), (37, 53, 1), (37, 53, 3),
          (64, 64, 2), (64, 64, 4)]


@pytest.mark.parametrize("h,w,r", SHAPES, ids=[f"{h}x{w}-r{r}" for h, w, r in SHAPES])
def test_tile_and_halo_shapes(h, w, r):
    depth, K, E, valid = _rough_case(h, w, seed=100 * h + w)
    min_pts = 3 if r == 1 else 6
    for vm, tag in ((valid, "holes"), (None, "all valid")):
        want = C.depth_normals(depth, K, E, valid=vm, radius=r, jump=0.01, min_pts=min_pts)
        _compare(_kernel(depth, K, E, valid=vm, radius=r, jump=0.01, min_pts=min_pts), want, f"{h}x{w} r={r} {tag}")
        if h * w > 2000 and vm is not None:
            break                                   # the large images once: the restatement is a Python loop
    if (h, w) == (3, 3):                            # the window is larger than the image: a clean plane, every pixel fits
        depth, K, E, _ = C.tilted_plane(3, 3, np.float32, f=60.0)
        want = C.depth_normals(depth, K, E, radius=r, jump=0.01, min_pts=3)
        assert want[1].all()
        _compare(_kernel(depth, K, E, radius=r, jump=0.01, min_pts=3), want, f"3x3 r={r} clean plane")


def test_bool_valid_map_and_other_parameters():
    depth, K, E, valid = _rough_case(20, 45, seed=9)
    d = torch.from_numpy(depth).cuda()
    Kt, Et = torch.from_numpy(K.astype(np.float32)), torch.from_numpy(E.astype(np.float32))
    a = ops.depth_normals(d, Kt, Et, valid=torch.from_numpy(valid).cuda(), radius=3, jump=0.03, min_pts=20)
    b = ops.depth_normals(d, Kt.cuda(), Et.cuda(), valid=torch.from_numpy(valid).cuda().bool(), radius=3, jump=0.03, min_pts=20)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _compare((a[0].cpu().numpy(), a[1].cpu().numpy()), C.depth_normals(depth, K, E, valid=valid, radius=3, jump=0.03, min_pts=20),
             "20x45 r=3 jump 0.03 min_pts 20")


def test_normals_face_the_camera_and_are_unit():
    for name in SCENES:
        sc = _scene(name)
        h, w = SCENES[name][1:3]
        ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
        for v in range(SCENES[name][0]):
            cam = sc["cams"][v].double().numpy()
            n, ok = _kernel(sc["depths"][v].numpy(), cam[1, :3, :3], cam[0])
            rays = np.linalg.inv(cam[1, :3, :3]) @ np.stack([xs, ys, np.ones_like(xs)]).reshape(3, -1)
            nc = cam[0, :3, :3] @ n.reshape(3, -1).astype(np.float64)
            dots = (nc * rays).sum(0)[ok.reshape(-1) > 0]
            norms = np.linalg.norm(n.astype(np.float64), axis=0)[ok > 0]
            print(f"{name} view {v}: largest nc . ray {dots.max():.3e}, |norm - 1| {np.abs(norms - 1).max():.2e}")
            assert (dots < 0).all()
            assert np.abs(norms - 1).max() <= 1e-6


def test_tilted_plane_on_the_gpu():
    depth, K, E, true_n = C.tilted_plane(24, 40, np.float32)
    n, ok = _kernel(depth, K, E)
    err = C.angle_deg(n.astype(np.float64), ok, true_n)
    print(f"tilted plane, float32 depths: max angle {err:.2e} deg")
    assert ok.all() and err < 5e-3                  # the float32 bound of tests/test_cloud_cpu.py


def test_rotating_the_world_rotates_the_normals():
    """E' = E with R' = R Q.  Q is a signed permutation, so R' is exact in float32 and the rotated normal has the same three
    products per component in another order: it may differ in the last float32 bit (1.2e-7 at 1.0), ok in nothing."""
    sc = _scene("s4x48x64")
    cam = sc["cams"][1].numpy()
    Q = np.array([[0, -1, 0], [0, 0, 1], [-1, 0, 0]], np.float32)
    assert np.isclose(np.linalg.det(Q), 1.0)
    E2 = cam[0].copy()
    E2[:3, :3] = cam[0][:3, :3] @ Q
    n1, ok1 = _kernel(sc["depths"][1].numpy(), cam[1, :3, :3], cam[0])
    n2, ok2 = _kernel(sc["depths"][1].numpy(), cam[1, :3, :3], E2)
    assert np.array_equal(ok1, ok2) and ok1.any()
    want = (Q.T.astype(np.float64) @ n1.reshape(3, -1).astype(np.float64)).reshape(n1.shape)
    assert np.abs(n2 - want).max() <= 1.2e-7


def test_invalid_arguments():
    d = torch.full((8, 9), 600.0, device="cuda")
    K, E = torch.eye(3), torch.eye(4)
    for kw in (dict(radius=0), dict(radius=5), dict(min_pts=2), dict(jump=0.0), dict(jump=-1.0), dict(jump=float("nan")),
               dict(radius=1, min_pts=10)):
        with pytest.raises(ValueError):
            ops.depth_normals(d, K, E, **kw)
    ops.depth_normals(d, K, E, radius=1, min_pts=9)
    lib = _lib.load()
    cam = torch.cat([K.reshape(9), E.reshape(16)]).contiguous()
    n, ok = torch.empty((3, 8, 9), device="cuda"), torch.empty((8, 9), dtype=torch.uint8, device="cuda")
    good = [d.data_ptr(), None, cam.data_ptr(), 8, 9, 2, 0.01, 6, n.data_ptr(), ok.data_ptr(), None]
    assert lib.cds_depth_normals_f32(*good) == 0
    for i in (0, 2, 8, 9):                          # depth, cam_host, normals, ok
        args = list(good)
        args[i] = None
        assert lib.cds_depth_normals_f32(*args) == _lib.EINVAL, i
    for i, val in ((3, 0), (4, 0)):                 # h, w
        args = list(good)
        args[i] = val
        assert lib.cds_depth_normals_f32(*args) == _lib.EINVAL, i
    torch.cuda.synchronize()
    # the merge: null pointers, more voxels than points
    p = torch.zeros((4, 3), device="cuda")
    c = torch.zeros(4, dtype=torch.int32, device="cuda")
    perm = torch.arange(4, device="cuda")
    start = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    op, oc, ok_ = torch.empty((1, 3), device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"), \
        torch.empty(1, dtype=torch.int32, device="cuda")
    good = [p.data_ptr(), c.data_ptr(), None, 4, perm.data_ptr(), start.data_ptr(), 1, op.data_ptr(), oc.data_ptr(), None,
            ok_.data_ptr(), None]
    assert lib.cds_voxel_merge_f32(*good) == 0
    for i in (0, 1, 4, 5, 7, 8, 10):
        args = list(good)
        args[i] = None
        assert lib.cds_voxel_merge_f32(*args) == _lib.EINVAL, i
    args = list(good)
    args[2] = p.data_ptr()                          # normals in, nowhere to write them
    assert lib.cds_voxel_merge_f32(*args) == _lib.EINVAL
    args = list(good)
    args[6] = 5
    assert lib.cds_voxel_merge_f32(*args) == _lib.EINVAL
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        pointcloud.merge_voxels(p, torch.zeros((4, 3), dtype=torch.uint8, device="cuda"), 0.0)
    with pytest.raises(ValueError):
        pointcloud.merge_voxels(p, torch.zeros((3, 3), dtype=torch.uint8, device="cuda"), 1.0)


# --------------------------------------------------------------------------------------------------------------- merge
@functools.lru_cache(maxsize=None)
def _scene_cloud():
    """Every pixel of every view of the second scene as a world point (float64 un-projection, rounded once), the image as
    its colour, and a seeded unit normal (every 50th is zero)."""
    sc = _scene("s4x48x64")
    n, h, w, _ = SCENES["s4x48x64"]
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)]).reshape(3, -1)
    pts = []
    for v in range(n):
        cam = sc["cams"][v].double().numpy()
        xc = np.linalg.inv(cam[1, :3, :3]) @ pix * sc["depths"][v].double().numpy().reshape(1, -1)
        pts.append((cam[0, :3, :3].T @ (xc - cam[0, :3, 3:4])).T)
    pts = np.concatenate(pts).astype(np.float32)
    col = (sc["imgs"].reshape(-1, 3) * 255).to(torch.uint8).numpy()
    rs = np.random.RandomState(11)
    nrm = rs.randn(len(pts), 3)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[::50] = 0
    return pts, col, nrm


def _merge_gpu(pts, col, voxel, nrm=None, **kw):
    m = pointcloud.merge_voxels(torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda(), voxel,
                                normals=None if nrm is None else torch.from_numpy(nrm).cuda(), **kw)
    assert m["points"].dtype == torch.float32 and m["colors"].dtype == torch.uint8 and m["counts"].dtype == torch.int32
    return m


def _compare_merge(m, want, what):
    assert np.array_equal(m["points"].cpu().numpy(), want["points"]), what
    assert np.array_equal(m["colors"].cpu().numpy(), want["colors"]), what
    assert np.array_equal(m["counts"].cpu().numpy(), want["counts"]), what
    if want["normals"] is None:
        assert m["normals"] is None
    else:
        err = float(np.abs(m["normals"].cpu().numpy().astype(np.float64) - want["normals"]).max()) if len(want["normals"]) else 0.0
        print(f"{what}: merged normals max-abs {err:.2e}")
        assert err <= NORMAL_TOL


@pytest.mark.parametrize("voxel", [30.0, 8.0])
def test_merge_vs_reference(voxel):
    pts, col, nrm = _scene_cloud()
    want = C.merge_voxels(pts, col, voxel, nrm)
    k = want["counts"]
    print(f"voxel {voxel}: {len(k)} voxels from {len(pts)} points, mean {k.mean():.1f}, max {k.max()}, "
          f"singletons {(k == 1).mean():.2f}")
    assert (k == 1).any() and (k > 1).any() and k.sum() == len(pts)
    m = _merge_gpu(pts, col, voxel, nrm)
    down, keys, counts = tt_eval.voxel_down_sample(torch.from_numpy(pts).cuda(), voxel, return_info=True)
    assert torch.equal(m["points"], down)                                 # the same bits, the same order
    assert np.array_equal(keys.cpu().numpy(), want["keys"]) and torch.equal(m["counts"].long(), counts)
    _compare_merge(m, want, f"voxel {voxel}")
    norms = m["normals"].double().norm(dim=1)
    assert bool((((norms - 1).abs() <= 1e-6) | (norms == 0)).all())
    # min_points = 2 drops exactly the singletons
    m2 = _merge_gpu(pts, col, voxel, nrm, min_points=2)
    multi = m["counts"] >= 2
    assert int(multi.sum()) == int((k > 1).sum()) < len(k)
    for key in ("points", "colors", "normals", "counts"):
        assert torch.equal(m2[key], m[key][multi]), key
    _compare_merge(m2, C.merge_voxels(pts, col, voxel, nrm, min_points=2), f"voxel {voxel} min_points 2")
    # without normals the rest is the same
    m3 = _merge_gpu(pts, col, voxel)
    assert m3["normals"] is None
    for key in ("points", "colors", "counts"):
        assert torch.equal(m3[key], m[key]), key
    # packed colours in: the same cloud
    m4 = pointcloud.merge_voxels(torch.from_numpy(pts).cuda(), pointcloud.pack_colors(torch.from_numpy(col).cuda()), voxel)
    assert torch.equal(m4["colors"], m["colors"])


def test_merge_edge_cases():
    pts, col, nrm = _scene_cloud()
    e = _merge_gpu(pts[:0], col[:0], 30.0, nrm[:0])
    assert tuple(e["points"].shape) == (0, 3) and tuple(e["colors"].shape) == (0, 3) and tuple(e["normals"].shape) == (0, 3) \
        and tuple(e["counts"].shape) == (0,)
    assert _merge_gpu(pts[:0], col[:0], 30.0)["normals"] is None
    _compare_merge(_merge_gpu(pts[:1], col[:1], 30.0, nrm[1:2]), C.merge_voxels(pts[:1], col[:1], 30.0, nrm[1:2]), "one point")
    one = _merge_gpu(pts[:1], col[:1], 30.0, nrm[1:2])
    assert np.array_equal(one["points"].cpu().numpy(), pts[:1]) and np.array_equal(one["colors"].cpu().numpy(), col[:1]) \
        and one["counts"].tolist() == [1]
    assert _merge_gpu(pts[:1], col[:1], 30.0, min_points=2)["points"].shape[0] == 0
    big = _merge_gpu(pts, col, 1e5, nrm)                                  # every point in one voxel
    assert big["counts"].tolist() == [len(pts)]
    _compare_merge(big, C.merge_voxels(pts, col, 1e5, nrm), "one voxel")
    # round half up, and normals that cancel
    p = np.zeros((2, 3), np.float32)
    c = np.array([[0, 1, 254], [1, 2, 255]], np.uint8)
    n = np.array([[0, 0, 1], [0, 0, -1]], np.float32)
    m = _merge_gpu(p, c, 1.0, n)
    assert m["colors"].tolist() == [[1, 2, 255]] and m["normals"].tolist() == [[0.0, 0.0, 0.0]]


# ------------------------------------------------------------------------------------------------------------- harness
def _write_outputs(tmp_path):
    from PIL import Image
    n, h, w, _ = SCENES["s4x48x64"]
    sc = _scene("s4x48x64")
    scan = tmp_path / "out" / "scan1"
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(scan / sub)
    for i in range(n):
        mvs_io.write_pfm(str(scan / "depth_est" / f"{i:08d}.pfm"), sc["depths"][i].numpy())
        mvs_io.write_pfm(str(scan / "confidence" / f"{i:08d}.pfm"), np.ascontiguousarray(sc["confs"][i].permute(1, 2, 0).numpy()))
        mvs_io.write_cam_file(str(scan / "cams" / f"{i:08d}_cam.txt"), sc["cams"][i].numpy())
        Image.fromarray((sc["imgs"][i].numpy() * 255).astype(np.uint8)).save(str(scan / "images" / f"{i:08d}.jpg"))
    pairs = tmp_path / "in" / "scan1"
    os.makedirs(pairs)
    with open(pairs / "pair.txt", "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            others = [j for j in range(n) if j != i]
            f.write(f"{i}\n{len(others)} " + " ".join(f"{j} 1.0" for j in others) + "\n")
    with open(tmp_path / "list.txt", "w") as f:
        f.write("scan1\n")
    return sc, scan, pairs


def _direct(sc, scan, method):
    """The kernels called directly: per view the fusion mask, ok of the normals, and the camera centre."""
    n = SCENES["s4x48x64"][0]
    th = torch.tensor(CONF).view(3, 1, 1)
    masks, oks, centres = [], [], []
    for i in range(n):
        others = [j for j in range(n) if j != i]
        cams = torch.stack([torch.from_numpy(fusion.read_fusion_cam(str(scan / "cams" / f"{j:08d}_cam.txt"))) for j in [i] + others])
        args = (sc["depths"][i].cuda(), sc["confs"][i].cuda(), cams[0], sc["depths"][others].cuda(), sc["confs"][others].cuda(),
                cams[1:])
        out = fusion.fuse_view_dynamic(*args, conf=CONF) if method == "dynamic" else fusion.fuse_view(*args, conf=CONF, thres_view=2)
        _, ok = ops.depth_normals(sc["depths"][i].cuda(), cams[0, 1, :3, :3], cams[0, 0], valid=(sc["confs"][i] > th).all(0).cuda())
        masks.append((out["mask"] > 0.5).cpu().numpy())
        oks.append(ok.cpu().numpy() > 0)
        E = cams[0, 0].double().numpy()
        centres.append(-E[:3, :3].T @ E[:3, 3])
    return masks, oks, centres


@pytest.mark.parametrize("method", ["normal", "dynamic"])
def test_filter_depth_harness(tmp_path, method):
    sc, scan, pairs = _write_outputs(tmp_path)
    kw = dict(conf=CONF, method=method, thres_view=2)
    out = tmp_path / "out"
    cli = ["--testpath", str(tmp_path / "in"), "--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--filter_method",
           method, "--conf", "0.1,0.1,0.1", "--thres_view", "2"]
    # without the new options: today's keys, the same bytes twice, today's reader
    plain = str(tmp_path / "plain.ply")
    info0 = fusion.filter_depth(str(pairs), str(scan), plain, **kw)
    assert set(info0) == {"points", "mean_final_mask"} | ({"admitted_at"} if method == "dynamic" else set())
    first = open(plain, "rb").read()
    fusion.filter_depth(str(pairs), str(scan), plain, **kw)
    assert open(plain, "rb").read() == first
    p0, c0 = fusion.read_ply(plain)
    assert p0.shape[0] == info0["points"] > 0 and c0.shape == p0.shape
    assert fusion.main(cli)["scan1"]["points"] == info0["points"] and open(out / "scan1.ply", "rb").read() == first
    # --normals
    masks, oks, centres = _direct(sc, scan, method)
    per_view = [int((m & o).sum()) for m, o in zip(masks, oks)]
    kept = sum(int(m.sum()) for m in masks)
    with_n = str(tmp_path / "normals.ply")
    info1 = fusion.filter_depth(str(pairs), str(scan), with_n, normals=True, **kw)
    p1, c1, n1 = fusion.read_ply_full(with_n)
    print(f"{method}: kept {kept}, with a normal {sum(per_view)} ({per_view}), no_normal {info1['no_normal']:.4f}")
    assert kept == info0["points"] and 0 < sum(per_view) < kept
    assert info1["points"] == p1.shape[0] == sum(per_view) and n1.shape == p1.shape == c1.shape
    assert abs(info1["no_normal"] - (kept - sum(per_view)) / kept) < 1e-12
    assert abs(info1["mean_final_mask"] - info0["mean_final_mask"]) < 1e-6
    assert np.abs(np.linalg.norm(n1.astype(np.float64), axis=1) - 1).max() <= 1e-6
    view = np.repeat(np.arange(len(per_view)), per_view)
    towards = np.stack(centres)[view] - p1.astype(np.float64)
    assert ((n1.astype(np.float64) * towards).sum(1) > 0).all()                  # every normal faces its view's camera
    # the kept points are those of the plain cloud that have a normal, colours included
    sel = np.concatenate([o[m] for m, o in zip(masks, oks)])
    assert np.array_equal(p1, p0[sel]) and np.array_equal(c1, c0[sel])
    assert np.array_equal(pointcloud.read_ply_points(with_n), p1)
    assert fusion.main(cli + ["--normals"])["scan1"] == info1 and open(out / "scan1.ply", "rb").read() == open(with_n, "rb").read()
    # --merge_voxel 30, without and with normals
    for normals, src, (ps, cs, ns) in ((False, plain, (p0, c0, None)), (True, with_n, (p1, c1, n1))):
        merged = str(tmp_path / f"merged{int(normals)}.ply")
        info2 = fusion.filter_depth(str(pairs), str(scan), merged, normals=normals, merge_voxel=30.0, **kw)
        p2, c2, n2 = fusion.read_ply_full(merged)
        m = pointcloud.merge_voxels(torch.from_numpy(ps).cuda(), torch.from_numpy(cs).cuda(), 30.0,
                                    normals=None if ns is None else torch.from_numpy(ns).cuda())
        assert np.array_equal(p2, m["points"].cpu().numpy()) and np.array_equal(c2, m["colors"].cpu().numpy())
        assert (n2 is None) == (not normals) and (n2 is None or np.array_equal(n2, m["normals"].cpu().numpy()))
        assert info2["points"] == p2.shape[0] < ps.shape[0] == info2["merged_from"]
        assert np.array_equal(tt_eval.read_ply_points(merged), p2)
        if not normals:
            assert np.array_equal(fusion.read_ply(merged)[0], p2)
    info3 = fusion.filter_depth(str(pairs), str(scan), str(tmp_path / "m2.ply"), normals=True, merge_voxel=30.0, merge_min_points=2,
                                **kw)
    assert info3["points"] == int((m["counts"] >= 2).sum()) < info2["points"]
    # the command line as a child process writes the same bytes
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "cds_mvsnet_amd.fusion"] + cli + ["--normals", "--merge_voxel", "30",
                                                                                 "--merge_min_points", "2"],
                         env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert f"scan1.ply: {info3['points']} points" in res.stdout and "no normal" in res.stdout and \
        f"merged from {info3['merged_from']}" in res.stdout
    assert open(out / "scan1.ply", "rb").read() == open(tmp_path / "m2.ply", "rb").read()


@pytest.mark.parametrize("method", ["normal", "dynamic"])
def test_filter_depth_is_the_views_in_pair_order(tmp_path, method):
    """The plain cloud, byte for byte: per reference view in pair.txt order the kept points of fuse_view / fuse_view_dynamic,
    row-major, with the colours of the uint8 image; and the call that only collects counts what the call that writes counts."""
    from PIL import Image
    sc, scan, pairs = _write_outputs(tmp_path)
    n = SCENES["s4x48x64"][0]
    pts, col, rates = [], [], []
    for i in range(n):
        others = [j for j in range(n) if j != i]
        cams = torch.stack([torch.from_numpy(fusion.read_fusion_cam(str(scan / "cams" / f"{j:08d}_cam.txt"))) for j in [i] + others])
        args = (sc["depths"][i].cuda(), sc["confs"][i].cuda(), cams[0], sc["depths"][others].cuda(), sc["confs"][others].cuda(),
                cams[1:])
        out = fusion.fuse_view_dynamic(*args, conf=CONF) if method == "dynamic" else fusion.fuse_view(*args, conf=CONF, thres_view=2)
        keep = (out["mask"] > 0.5).cpu().numpy()
        img = np.asarray(Image.open(str(scan / "images" / f"{i:08d}.jpg")).convert("RGB"))
        assert img.dtype == np.uint8 and img.shape == keep.shape + (3,)
        pts.append(out["points"].cpu().numpy()[:, keep].T)
        col.append(img[keep])
        rates.append(keep.sum() / keep.size)
    want = str(tmp_path / "assembled.ply")
    fusion.write_ply(want, np.concatenate(pts), np.concatenate(col))
    kw = dict(conf=CONF, method=method, thres_view=2)
    plain = str(tmp_path / "plain.ply")
    info = fusion.filter_depth(str(pairs), str(scan), plain, **kw)
    print(f"{method}: {info['points']} points, mean_final_mask {info['mean_final_mask']!r}, per view {[len(p) for p in pts]}")
    assert info["points"] == sum(len(p) for p in pts) > 0 and all(len(p) > 0 for p in pts)
    assert open(plain, "rb").read() == open(want, "rb").read()
    assert info["mean_final_mask"] == float(np.mean(np.array(rates, np.float64)))
    views = []
    counted = fusion.filter_depth(str(pairs), str(scan), None, collect=views, **kw)
    assert counted == info
    assert len(views) == n and all(v["image"].dtype == torch.uint8 for v in views)
    assert np.array_equal(torch.cat([v["points"] for v in views]).cpu().numpy(), np.concatenate(pts))
    assert np.array_equal(torch.cat([v["image"][v["mask"]] for v in views]).cpu().numpy(), np.concatenate(col))


def test_infer_fuse_normals_merge(tmp_path, capsys):
    """infer --fuse --normals --merge_voxel end to end on the tiny synthetic scan of test_infer_fuse_dynamic (an untrained
    network: loose consistency settings, a wide jump)."""
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanA", 4, 128, 160, seed=3)
    with open(tmp_path / "list.txt", "w") as f:
        f.write("scanA\n")
    out = str(tmp_path / "out")
    infer.main(["--testpath", root, "--testlist", str(tmp_path / "list.txt"), "--outdir", out, "--num_view", "3",
                "--max_h", "128", "--max_w", "160", "--interval_scale", "1.0", "--fuse", "--filter_method", "dynamic",
                "--conf", "0.0,0.0,0.0", "--dyn_dist_base", "2.0", "--dyn_rel_base", "0.02", "--dyn_views", "1,10",
                "--normals", "--normal_jump", "0.05", "--merge_voxel", "10"])
    pts, col, nrm = fusion.read_ply_full(os.path.join(out, "scanA.ply"))
    assert pts.shape[0] > 0 and pts.shape == col.shape == nrm.shape and np.isfinite(pts).all()
    norms = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert ((np.abs(norms - 1) <= 1e-6) | (norms == 0)).all() and (norms > 0).any()
    line = [ln for ln in capsys.readouterr().out.splitlines() if "scanA.ply" in ln]
    assert line and f"{pts.shape[0]} points" in line[0] and "no normal" in line[0] and "merged from" in line[0]
