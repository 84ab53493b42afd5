"""The weighted integration of csrc/tsdf.hip (cds_tsdf_view_weights, cds_tsdf_integrate_w_f32) against the numpy
restatement of its rule (mesh_weighted_ref.py), the extraction of a weighted volume, and the way of the options through
mesh_views, mesh_scan and the command line."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_ref as M
import mesh_weighted_ref as W
from cds_mvsnet_amd import _lib, infer, mesh, mvs_io, ops, synth
from test_mvs_io import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACC = ("sum", "n", "nc", "rgb")


def _cuda(sc, wt=None):
    out = [torch.from_numpy(sc[k]).cuda() for k in ("depths", "masks", "images")] + [torch.from_numpy(sc["cams"])]
    return out, (torch.from_numpy(wt).cuda() if wt is not None else None)


def _integrate_gpu(sc, trunc_voxels, wt=None, **kw):
    args, weights = _cuda(sc, wt)
    t = mesh.TsdfVolume(torch.from_numpy(sc["points"]).cuda(), sc["voxel"], trunc_voxels * sc["voxel"])
    t.integrate(*args, weights=weights, **kw)
    return t


# ---------------------------------------------------------------------------------------------------------- 6. weight maps
def _conf_map(h, w, seed):
    rs = np.random.RandomState(900 + seed)
    conf = rs.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    for bad in (np.nan, -0.25, 1.5, np.inf, 0.0):
        conf[rs.randint(0, h, 40), rs.randint(0, w, 40)] = bad
    return conf


@pytest.mark.parametrize("mode", ["angle", "conf", "angle_conf"])
def test_view_weights_vs_restatement(mode):
    """Views 0..5 of integration_scene (37 x 50; two of them look along the plane): the kernel's map equals the restatement's
    for the normals that ops.depth_normals gives it; conf holds NaN, negative, > 1 and infinite entries."""
    sc = M.integration_case(33, 4.0)[0]
    seen = np.zeros(256, np.int64)
    for v in range(6):
        depth, msk, cam = sc["depths"][v], sc["masks"][v], sc["cams"][v]
        d, m = torch.from_numpy(depth).cuda(), torch.from_numpy(msk).cuda()
        conf = _conf_map(*depth.shape, v) if mode != "angle" else None
        nrm = ok = None
        if mode != "conf":
            nrm, ok = (x.cpu().numpy() for x in ops.depth_normals(d, cam[1, :3, :3], cam[0], valid=m))
            assert 0 < ok.sum() < (msk != 0).sum()
        want = W.view_weights(depth, msk, cam[1, :3, :3], cam[0], nrm, ok, conf)
        got = mesh.view_weights(d, m, torch.from_numpy(cam), torch.from_numpy(conf).cuda() if conf is not None else None, mode=mode)
        assert got.dtype == torch.uint8 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), f"view {v}: {(got.cpu().numpy() != want).sum()} pixels differ"
        seen += np.bincount(want.reshape(-1), minlength=256)
    print(f"{mode}: {seen[0]} pixels weigh 0, {seen[1]} weigh 1, {seen[2:255].sum()} weigh 2..254, {seen[255]} weigh 255")
    assert seen[0] > 0 and seen[1] > 0 and seen[2:255].sum() > 0 and (mode == "angle" or seen[255] > 0)


def test_view_weights_arguments():
    sc = M.integration_case(33, 4.0)[0]
    d, m, cam = torch.from_numpy(sc["depths"][0]).cuda(), torch.from_numpy(sc["masks"][0]).cuda(), torch.from_numpy(sc["cams"][0])
    for mode in ("conf", "angle_conf"):
        with pytest.raises(ValueError, match="needs conf"):
            mesh.view_weights(d, m, cam, mode=mode)
    with pytest.raises(ValueError, match="mode must be"):
        mesh.view_weights(d, m, cam, mode="one")
    with pytest.raises(RuntimeError):
        mesh.view_weights(d.cpu(), m, cam)
    bad = cam.clone()
    bad[1, 2, 0] = 1e-3                                             # a last row of K that is not (0, 0, 1)
    with pytest.raises(ValueError, match="intrinsic"):
        mesh.view_weights(d, m, bad)
    # the C entry point refuses what the wrapper never sends
    lib = _lib.load()
    h, w = d.shape
    out = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    host = torch.cat([bad[1, :3, :3].reshape(9), bad[0].reshape(16)]).contiguous()
    good = torch.cat([cam[1, :3, :3].reshape(9), cam[0].reshape(16)]).contiguous()
    nrm = torch.zeros((3, h, w), device="cuda")
    assert lib.cds_tsdf_view_weights(d.data_ptr(), m.data_ptr(), None, None, None, host.data_ptr(), h, w, out.data_ptr(), None) == _lib.EINVAL
    assert lib.cds_tsdf_view_weights(d.data_ptr(), m.data_ptr(), nrm.data_ptr(), None, None, good.data_ptr(), h, w, out.data_ptr(),
                                     None) == _lib.EINVAL           # normals without ok
    assert lib.cds_tsdf_view_weights(d.data_ptr(), m.data_ptr(), None, None, None, good.data_ptr(), 0, w, out.data_ptr(), None) == _lib.EINVAL
    assert int(out.sum()) == 0


# ----------------------------------------------------------------------------------------------------------- 7. integration
def _compare_volume(t, vol, what):
    """Block set, n, wn, nc and the colour sums exactly; sum within n 2^-24 max(1, wn): n adds, each rounding a partial sum of
    magnitude at most wn (bit-equal is expected)."""
    assert np.array_equal(t.keys.cpu().numpy(), vol["keys"]), f"{what}: allocated blocks differ"
    for name in ("n", "nc", "rgb"):
        assert np.array_equal(getattr(t, name).cpu().numpy(), vol[name]), f"{what}: {name} differs"
    if t.wn is None:
        assert np.array_equal(vol["wn"], vol["n"])
    else:
        assert np.array_equal(t.wn.cpu().numpy(), vol["wn"]), f"{what}: wn differs"
    got = t.sum.cpu().numpy()
    diff = np.abs(got.astype(np.float64) - vol["sum"].astype(np.float64))
    bound = vol["n"] * 2.0 ** -24 * np.maximum(1.0, vol["wn"])
    print(f"{what}: {len(vol['keys'])} blocks, n up to {vol['n'].max()}, wn up to {vol['wn'].max()}, largest sum difference "
          f"{diff.max():.3g}, bit-equal {np.array_equal(got, vol['sum'])}")
    assert (diff <= bound).all(), f"{what}: sum off by {diff.max()}"


def test_the_scene_reaches_every_path_of_the_interpolation():
    """On the reference alone: of all quads of the 33 maps, those that interpolate, those with a corner that is not kept and those
    that the jump test rejects are each at least 5 %."""
    sc = M.integration_case(33, 4.0)[0]
    state = np.stack([W.quad_state(sc["depths"][v], sc["masks"][v], W.JUMP) for v in range(33)])
    share = [float((state == k).mean()) for k in range(3)]
    print("quads: {:.1f} % interpolate, {:.1f} % have a corner that is not kept, {:.1f} % fail the jump test".format(
        *(100 * s for s in share)))
    assert min(share) >= 0.05


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("interp", [False, True])
@pytest.mark.parametrize("n_views,trunc_voxels", [(1, 4.0), (32, 4.0), (33, 1.0), (33, 8.0), (70, 4.0)])
def test_integration_vs_restatement(n_views, trunc_voxels, interp, weighted):
    """The cases of test_mesh_gpu.test_integration_vs_restatement (one view, a full chunk, one more, two chunks and a remainder;
    T = s and T = 8 s), nearest and interpolated depth, without weights and with a map a quarter of which is 0."""
    sc, wt, vol = W.integration_case(n_views, trunc_voxels, weighted, interp)
    assert vol["n"].max() > 0 and (vol["n"] == 0).any() and (vol["nc"] < vol["n"]).any()
    if weighted:
        assert (vol["wn"] > vol["n"]).any()
    t = _integrate_gpu(sc, trunc_voxels, wt, interp=interp, interp_jump=W.JUMP)
    assert (t.wn is not None) == weighted
    _compare_volume(t, vol, f"V = {n_views}, T = {trunc_voxels} s, interp {interp}, weights {weighted}")


# ---------------------------------------------------------------------------------------------------------------- 8. chunks
def test_weighted_integration_does_not_depend_on_the_chunk():
    sc, wt, vol = W.integration_case(33, 8.0, True, True)
    a = _integrate_gpu(sc, 8.0, wt, interp=True, chunk=1)
    b = _integrate_gpu(sc, 8.0, wt, interp=True, chunk=32)
    for name in ACC + ("wn",):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # views added in two calls are the same as in one
    args, weights = _cuda(sc, wt)
    c = mesh.TsdfVolume(torch.from_numpy(sc["points"]).cuda(), sc["voxel"], 8.0 * sc["voxel"])
    c.integrate(*[x[:5] for x in args], weights=weights[:5], interp=True)
    c.integrate(*[x[5:] for x in args], weights=weights[5:], interp=True)
    for name in ACC + ("wn",):
        assert torch.equal(getattr(c, name), getattr(a, name)), name


def test_weighted_and_unweighted_views_do_not_mix():
    sc, wt, _ = W.integration_case(1, 4.0, True, False)
    args, weights = _cuda(sc, wt)
    t = mesh.TsdfVolume(torch.from_numpy(sc["points"]).cuda(), sc["voxel"])
    t.integrate(*args, weights=weights)
    with pytest.raises(ValueError, match="do not mix"):
        t.integrate(*args)
    u = mesh.TsdfVolume(torch.from_numpy(sc["points"]).cuda(), sc["voxel"])
    u.integrate(*args, interp=True)                                 # interpolation alone leaves the volume unweighted
    u.integrate(*args)
    assert u.wn is None
    with pytest.raises(ValueError, match="do not mix"):
        u.integrate(*args, weights=weights)
    with pytest.raises(ValueError, match="weights must be uint8"):
        u.integrate(*args, weights=weights.float())
    with pytest.raises(ValueError, match="interp_jump must be positive"):
        u.integrate(*args, interp=True, interp_jump=0.0)
    with pytest.raises(RuntimeError):
        t.integrate(*args, weights=weights.cpu())


# ------------------------------------------------------------------------------------------------------- 9. the old kernel
def test_without_weights_and_interpolation_the_new_kernel_gives_the_old_bits():
    sc = M.integration_case(33, 8.0)[0]
    old = _integrate_gpu(sc, 8.0)
    args, _ = _cuda(sc)
    depths, masks, images, cams = args
    v, h, w = depths.shape
    new = mesh.TsdfVolume(torch.from_numpy(sc["points"]).cuda(), sc["voxel"], 8.0 * sc["voxel"])
    cam = cams.double().cuda()
    ok = (masks != 0) & torch.isfinite(depths) & (depths > 0)
    tab = torch.zeros((v, 24), dtype=torch.float64, device="cuda")
    tab[:, 0:9], tab[:, 9:12], tab[:, 12:21] = cam[:, 0, :3, :3].reshape(v, 9), cam[:, 0, :3, 3], cam[:, 1, :3, :3].reshape(v, 9)
    tab[:, 21] = torch.where(ok, depths, torch.full_like(depths, -math.inf)).flatten(1).amax(1).double()
    lib, hw = _lib.load(), h * w
    base = [new.keys.data_ptr(), new.n_blocks, new._frame.data_ptr(), new._dims.data_ptr(), new.trunc]
    acc = [new.sum.data_ptr(), new.n.data_ptr(), new.nc.data_ptr(), new.rgb.data_ptr()]
    wn = torch.zeros_like(new.n)
    wt = torch.ones((v, h, w), dtype=torch.uint8, device="cuda")
    for v0, nv in ((0, 32), (32, 1)):
        maps = [depths.data_ptr() + 4 * v0 * hw, masks.data_ptr() + v0 * hw, images.data_ptr() + 3 * v0 * hw,
                tab.data_ptr() + 8 * 24 * v0]
        # weights without wn, wn without weights, an interpolation without a usable jump: refused, nothing written
        assert lib.cds_tsdf_integrate_w_f32(*base, *maps, nv, h, w, *acc, wt.data_ptr(), 0, 0.05, None, None) == _lib.EINVAL
        assert lib.cds_tsdf_integrate_w_f32(*base, *maps, nv, h, w, *acc, None, 0, 0.05, wn.data_ptr(), None) == _lib.EINVAL
        for jump in (0.0, -1.0, math.nan, math.inf):
            assert lib.cds_tsdf_integrate_w_f32(*base, *maps, nv, h, w, *acc, None, 1, jump, None, None) == _lib.EINVAL
        assert lib.cds_tsdf_integrate_w_f32(*base, *maps, 33, h, w, *acc, None, 0, 0.05, None, None) == _lib.EINVAL
        assert lib.cds_tsdf_integrate_w_f32(*base, *maps, nv, h, w, *acc, None, 0, 0.0, None, None) == 0
    torch.cuda.synchronize()
    assert int(old.n.max()) > 1
    for name in ACC:
        assert torch.equal(getattr(new, name), getattr(old, name)), name
    assert int(wn.sum()) == 0


# ------------------------------------------------------------------------------------------------------------ 10. extraction
def _upload(vol):
    t = mesh.TsdfVolume.from_blocks(vol["origin"], vol["voxel"], vol["trunc"], vol["nb"], vol["keys"])
    for name in ACC:
        getattr(t, name).copy_(torch.from_numpy(vol[name]))
    t.wn = torch.from_numpy(vol["wn"]).cuda()
    return t


def _compare_mesh(got, want, what):
    """faces, vertex count and colours identical; positions within 2 ulp of fp32 (the bar of test_mesh_gpu.py)."""
    v, c, f = got["vertices"].cpu().numpy(), got["colors"].cpu().numpy(), got["faces"].cpu().numpy()
    assert v.shape == want["vertices"].shape and f.shape == want["faces"].shape, \
        f"{what}: {v.shape[0]} vertices / {f.shape[0]} faces, expected {want['vertices'].shape[0]} / {want['faces'].shape[0]}"
    assert np.array_equal(f, want["faces"]), f"{what}: faces differ"
    assert np.array_equal(c, want["colors"]), f"{what}: colours differ"
    err = np.abs(v.astype(np.float64) - want["vertices"].astype(np.float64)) / np.spacing(np.abs(want["vertices"]))
    print(f"{what}: {v.shape[0]} vertices, {f.shape[0]} faces, largest position difference {err.max() if err.size else 0.0:.2f} ulp")
    assert err.size == 0 or err.max() <= 2.0, f"{what}: a position {err.max()} ulp off"


@pytest.mark.parametrize("min_weight", [1, 2, 4])
def test_extraction_of_a_weighted_volume(min_weight):
    """Validity counts views (n), the distance divides by the weights (wn): the mesh of the restatement, which differs from the
    one that divides by n."""
    vol = W.integration_case(33, 4.0, True, True)[2]
    want = W.extract(vol, min_weight)
    assert len(want["faces"]) > 0
    t = _upload(vol)
    _compare_mesh(t.extract(min_weight), want, f"min_weight {min_weight}")
    t.wn = None
    by_n = t.extract(min_weight)
    assert by_n["faces"].shape == want["faces"].shape and not np.array_equal(by_n["vertices"].cpu().numpy(), want["vertices"])


# ------------------------------------------------------------------------------------------------------------ 11. end to end
def _sphere_records():
    """Records as filter_depth(collect=...) gathers them, from mesh_ref.sphere_scene."""
    sc = M.sphere_case()[0]
    counts = [int((m != 0).sum()) for m in sc["masks"]]
    pts = np.split(sc["points"], np.cumsum(counts)[:-1])
    views = [{"depth": torch.from_numpy(sc["depths"][v]).cuda(), "mask": torch.from_numpy(sc["masks"][v] != 0).cuda(),
              "image": torch.from_numpy(sc["images"][v]).cuda(), "cam": torch.from_numpy(sc["cams"][v]),
              "points": torch.from_numpy(pts[v]).cuda(), "conf": torch.full(sc["depths"][v].shape, 0.5, device="cuda")}
             for v in range(len(counts))]
    return sc, views


def test_mesh_views_end_to_end():
    """The 26-camera sphere through mesh_views: angle weights and interpolation give a closed mesh whose rms radial error is at
    most half that of the default path on the same device (the bar of test_mesh_weighted_cpu.test_sphere_error_by_mode); with
    default arguments the mesh has the bytes of TsdfVolume(...).integrate(...).extract(...)."""
    sc, views = _sphere_records()
    s = sc["voxel"]
    plain, vol0 = mesh.mesh_views(views, s, 2.5 * s, 2)
    both, vol1 = mesh.mesh_views(views, s, 2.5 * s, 2, weight="angle", interp=True)
    assert vol0.wn is None and vol1.wn is not None and int(vol1.wn.max()) > int(vol1.n.max())
    t = mesh.TsdfVolume(torch.from_numpy(sc["points"]).cuda(), s, 2.5 * s)
    t.integrate(*_cuda(sc)[0])
    direct = t.extract(2)
    for k in ("vertices", "colors", "faces"):
        assert torch.equal(plain[k], direct[k]), k
    err = {}
    for name, m in (("one", plain), ("angle + interp", both)):
        v, f = m["vertices"].cpu().numpy(), m["faces"].cpu().numpy()
        tp = M.topology(f, len(v))
        assert tp["euler"] == 2 and (tp["edge_uses"] == 2).all() and tp["directed_unique"] and tp["reverse_present"], name
        err[name] = W.radial_error(v, sc)
        print(f"{name}: rms {err[name][0]:.4f}, max {err[name][1]:.4f} voxels, {len(v)} vertices, {len(f)} faces")
    assert err["angle + interp"][0] <= 0.5 * err["one"][0]
    assert err["angle + interp"][1] < err["one"][1]
    # a constant confidence of 0.5 halves every weight (up to its rounding): another volume, nearly the same surface
    conf, vol2 = mesh.mesh_views(views, s, 2.5 * s, 2, weight="angle_conf", interp=True)
    assert not torch.equal(vol2.wn, vol1.wn) and torch.equal(vol2.n, vol1.n)
    assert W.radial_error(conf["vertices"].cpu().numpy(), sc)[0] <= 0.5 * err["one"][0]
    with pytest.raises(ValueError, match="weight must be one of"):
        mesh.mesh_views(views, s, weight="cosine")
    with pytest.raises(ValueError, match="needs conf"):
        mesh.mesh_views([{k: x for k, x in v.items() if k != "conf"} for v in views], s, weight="conf")


# --------------------------------------------------------------------------------------------------------- 12. command line
VOXEL = 16.0


def _write_scan(tmp_path, n=4, h=37, w=50):
    """synth.make_fusion_scene(4, 37, 50) in the layout infer writes: <out>/scan1/{depth_est,confidence,cams,images}."""
    from PIL import Image
    sc = synth.make_fusion_scene(n, h, w)
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
    return scan, pairs


def test_command_line(tmp_path, capsys):
    """Four saved views of 37 x 50: --mesh_weight angle --mesh_interp through the command line as a child process writes the
    mesh of mesh_scan(weight="angle", interp=True), which is not the default one; the conf modes read the saved confidence; the
    options are refused where no volume is integrated."""
    scan, pairs = _write_scan(tmp_path)
    out = tmp_path / "out"
    kw = dict(thres_view=1)
    files = {}
    for name, opts in (("one", {}), ("angle", dict(weight="angle", interp=True)), ("conf", dict(weight="angle_conf")),
                       ("jump", dict(weight="angle", interp=True, interp_jump=1e-4))):
        files[name] = str(tmp_path / f"{name}_mesh.ply")
        info = mesh.mesh_scan(str(pairs), str(scan), files[name], VOXEL, **opts, **kw)
        assert info["vertices"] > 0 and info["faces"] > 0, name
    data = {k: open(p, "rb").read() for k, p in files.items()}
    assert len(set(data.values())) == 4
    cli = ["--testpath", str(tmp_path / "in"), "--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--thres_view", "1",
           "--mesh_voxel", str(VOXEL)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "cds_mvsnet_amd.mesh"] + cli + ["--mesh_weight", "angle", "--mesh_interp"], env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert open(out / "scan1_mesh.ply", "rb").read() == data["angle"]
    os.remove(out / "scan1_mesh.ply")
    mesh.main(cli + ["--mesh_weight", "angle", "--mesh_interp", "--mesh_interp_jump", "1e-4"])
    assert open(out / "scan1_mesh.ply", "rb").read() == data["jump"]
    mesh.main(cli)
    assert open(out / "scan1_mesh.ply", "rb").read() == data["one"]
    capsys.readouterr()
    for argv in (["--from_mesh", files["one"], "--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--mesh_weight", "angle"],
                 ["--from_mesh", files["one"], "--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--mesh_interp"],
                 ["--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--mesh_weight", "conf"]):
        with pytest.raises(SystemExit):
            mesh.main(argv)
        assert "--mesh_voxel" in capsys.readouterr().err
    with pytest.raises(ValueError, match="weight must be one of"):
        mesh.mesh_scan(str(pairs), str(scan), str(tmp_path / "x_mesh.ply"), VOXEL, weight="two", **kw)
    assert not (tmp_path / "x_mesh.ply").exists()


def test_infer_fuse_passes_the_options(tmp_path, capsys):
    """infer --fuse --mesh_voxel --mesh_weight angle_conf --mesh_interp on the scene of test_mesh_gpu.test_infer_fuse_mesh (3 views
    of 128 x 160, an untrained network): the mesh of mesh_scan with the same options on the depth maps infer saved, and not the
    default one."""
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanA", 3, 128, 160, seed=3)
    with open(tmp_path / "list.txt", "w") as f:
        f.write("scanA\n")
    out = str(tmp_path / "out")
    infer.main(["--testpath", root, "--testlist", str(tmp_path / "list.txt"), "--outdir", out, "--num_view", "3", "--max_h", "128",
                "--max_w", "160", "--interval_scale", "1.0", "--fuse", "--mesh_voxel", "10", "--filter_method", "dynamic", "--conf",
                "0.0,0.0,0.0", "--dyn_dist_base", "2.0", "--dyn_rel_base", "0.02", "--dyn_views", "1,10", "--mesh_weight", "angle_conf",
                "--mesh_interp", "--mesh_interp_jump", "0.1"])
    assert [ln for ln in capsys.readouterr().out.splitlines() if "scanA_mesh.ply" in ln and "faces" in ln]
    via_infer = open(os.path.join(out, "scanA_mesh.ply"), "rb").read()
    kw = dict(method="dynamic", conf=(0.0, 0.0, 0.0), dist_base=2.0, rel_base=0.02, n_views=(1, 10))
    same, plain = str(tmp_path / "same_mesh.ply"), str(tmp_path / "plain_mesh.ply")
    info = mesh.mesh_scan(os.path.join(root, "scanA"), os.path.join(out, "scanA"), same, 10.0, weight="angle_conf", interp=True,
                          interp_jump=0.1, **kw)
    mesh.mesh_scan(os.path.join(root, "scanA"), os.path.join(out, "scanA"), plain, 10.0, **kw)
    assert info["faces"] > 0 and open(same, "rb").read() == via_infer != open(plain, "rb").read()
