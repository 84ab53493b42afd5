"""The TSDF kernels of csrc/tsdf.hip against the numpy restatement of their rule (mesh_ref.py), and the way from
saved depth maps to a mesh file through mesh_scan, the command line and infer --fuse."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_ref as M
from cds_mvsnet_amd import _lib, fusion, infer, mesh, mvs_io, pointcloud, synth
from test_mvs_io import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _upload(vol):
    """A restatement volume as a TsdfVolume with the same accumulators."""
    t = mesh.TsdfVolume.from_blocks(vol["origin"], vol["voxel"], vol["trunc"], vol["nb"], vol["keys"])
    assert np.array_equal(t.keys.cpu().numpy(), vol["keys"])
    for name in ("sum", "n", "nc", "rgb"):
        getattr(t, name).copy_(torch.from_numpy(vol[name]))
    return t


def _compare_mesh(got, want, what):
    """faces, vertex count and colours identical; positions within 2 ulp of fp32 at the coordinate's magnitude (both sides
    round one fp64 value once; the allowance is for numpy's operation order in Xa + tt (Xb - Xa))."""
    v, c, f = got["vertices"].cpu().numpy(), got["colors"].cpu().numpy(), got["faces"].cpu().numpy()
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32
    assert v.shape == want["vertices"].shape and f.shape == want["faces"].shape, \
        f"{what}: {v.shape[0]} vertices / {f.shape[0]} faces, expected {want['vertices'].shape[0]} / {want['faces'].shape[0]}"
    assert np.array_equal(f, want["faces"]), f"{what}: faces differ"
    assert np.array_equal(c, want["colors"]), f"{what}: colours differ"
    ulp = np.spacing(np.abs(want["vertices"]))
    err = np.abs(v.astype(np.float64) - want["vertices"].astype(np.float64)) / ulp
    print(f"{what}: {v.shape[0]} vertices, {f.shape[0]} faces, largest position difference {err.max() if err.size else 0.0:.2f} ulp")
    assert err.size == 0 or err.max() <= 2.0, f"{what}: a position {err.max()} ulp off"


# ------------------------------------------------------------------------------------------------------------- extraction
@pytest.mark.parametrize("name", ["sphere", "aligned", "hole"])
def test_extraction_vs_restatement(name):
    vol, want = M.analytic_case(name)
    assert len(want["faces"]) > 0
    _compare_mesh(_upload(vol).extract(2), want, name)


def test_extraction_weight_threshold_and_empty():
    vol, want = M.analytic_case("sphere")
    t = _upload(vol)
    for mw in (1, 2):
        _compare_mesh(t.extract(mw), want, f"min_weight {mw}")
    out = t.extract(3)                                             # every point was seen twice: nothing is valid
    assert out["vertices"].shape == (0, 3) and out["colors"].shape == (0, 3) and out["faces"].shape == (0, 3)
    t.n[4] = 1                                                     # block (1, 1, 0) seen once: the mesh of the missing block
    _compare_mesh(t.extract(2), M.analytic_case("hole")[1], "one block under the threshold")
    with pytest.raises(ValueError):
        t.extract(0)


# ------------------------------------------------------------------------------------------------------------ integration
def _integrate_gpu(sc, trunc_voxels, **kw):
    t = mesh.TsdfVolume(torch.from_numpy(sc["points"]).cuda(), sc["voxel"], trunc_voxels * sc["voxel"])
    t.integrate(torch.from_numpy(sc["depths"]).cuda(), torch.from_numpy(sc["masks"]).cuda(), torch.from_numpy(sc["images"]).cuda(),
                torch.from_numpy(sc["cams"]), **kw)
    return t


def _compare_volume(t, vol, what):
    """Frame, block set, n, nc and the colour sums exactly; sum within n 2^-24 max(1, |sum|) (bit-equal is expected)."""
    assert np.array_equal(t.origin, vol["origin"]) and t.nb.tolist() == vol["nb"].tolist()
    assert np.array_equal(t.keys.cpu().numpy(), vol["keys"]), f"{what}: allocated blocks differ"
    assert np.array_equal(t.table.cpu().numpy().reshape(-1)[vol["keys"]], np.arange(len(vol["keys"])))
    assert int((t.table >= 0).sum()) == len(vol["keys"])
    for name in ("n", "nc", "rgb"):
        assert np.array_equal(getattr(t, name).cpu().numpy(), vol[name]), f"{what}: {name} differs"
    got = t.sum.cpu().numpy()
    diff = np.abs(got.astype(np.float64) - vol["sum"].astype(np.float64))
    bound = vol["n"] * 2.0 ** -24 * np.maximum(1.0, np.abs(vol["sum"].astype(np.float64)))
    print(f"{what}: {len(vol['keys'])} blocks, n up to {vol['n'].max()}, largest sum difference {diff.max():.3g}, "
          f"bit-equal {np.array_equal(got, vol['sum'])}")
    assert (diff <= bound).all(), f"{what}: sum off by {diff.max()}"


@pytest.mark.parametrize("n_views,trunc_voxels", [(1, 4.0), (32, 4.0), (33, 1.0), (33, 8.0), (70, 4.0)])
def test_integration_vs_restatement(n_views, trunc_voxels):
    """50 x 37 maps (no multiple of the wave), one view, a full chunk of 32, one more, two chunks and a remainder; T = s and
    T = 8 s; lattice points behind a camera and outside the map; masked pixels and depths 0, NaN, +-inf, negative; the allocated
    blocks fill the block grid to its border."""
    sc, vol = M.integration_case(n_views, trunc_voxels)
    assert mesh.CHUNK_VIEWS == 32
    b = vol["keys"] % vol["nb"][0]
    assert b.min() == 0 and b.max() == vol["nb"][0] - 1                                    # blocks on the border of the grid
    assert vol["n"].max() > 0 and (vol["n"] == 0).any() and (vol["nc"] < vol["n"]).any()
    _compare_volume(_integrate_gpu(sc, trunc_voxels), vol, f"V = {n_views}, T = {trunc_voxels} s")


def test_integration_does_not_depend_on_the_chunk():
    sc, vol = M.integration_case(33, 8.0)
    a = _integrate_gpu(sc, 8.0, chunk=1)
    b = _integrate_gpu(sc, 8.0, chunk=16)
    _compare_volume(a, vol, "one view per launch")
    for name in ("sum", "n", "nc", "rgb"):
        assert torch.equal(getattr(a, name), getattr(b, name))
    # views added in two calls are the same as in one
    c = mesh.TsdfVolume(torch.from_numpy(sc["points"]).cuda(), sc["voxel"], 8.0 * sc["voxel"])
    args = [torch.from_numpy(sc[k]).cuda() for k in ("depths", "masks", "images")] + [torch.from_numpy(sc["cams"])]
    c.integrate(*[x[:5] for x in args])
    c.integrate(*[x[5:] for x in args])
    assert torch.equal(c.sum, a.sum) and torch.equal(c.n, a.n) and torch.equal(c.rgb, a.rgb)
    # a float mask and a bool mask mean the same
    d = mesh.TsdfVolume(torch.from_numpy(sc["points"]).cuda(), sc["voxel"], 8.0 * sc["voxel"])
    d.integrate(args[0], args[1].float(), args[2], args[3])
    assert torch.equal(d.sum, a.sum) and torch.equal(d.nc, a.nc)


# ----------------------------------------------------------------------------------------------------------- sphere scene
def _sphere_gpu():
    sc, _, _ = M.sphere_case()
    t = _integrate_gpu(sc, 2.5)
    return t, t.extract(2)


def test_sphere_scene():
    """The 26-camera sphere of test_mesh_cpu.test_sphere_scene_restatement: the GPU mesh equals the restatement's, and distance
    and volume stay within the restatement's measured values (0.40666 voxel, 1.01630) plus 25 %."""
    sc, vol, want = M.sphere_case()
    t, got = _sphere_gpu()
    _compare_volume(t, vol, "sphere scene")
    _compare_mesh(got, want, "sphere scene")
    v, f = got["vertices"].cpu().numpy().astype(np.float64), got["faces"].cpu().numpy()
    tp = M.topology(f, len(v))
    assert (tp["edge_uses"] == 2).all() and tp["directed_unique"] and tp["reverse_present"] and tp["euler"] == 2
    r, s = sc["radius"], sc["voxel"]
    ratio = M.signed_volume(v - sc["centre"], f) / (4.0 / 3.0 * np.pi * r ** 3)
    dist = (np.abs(np.linalg.norm(v - sc["centre"], axis=1) - r) / s).max()
    print(f"volume ratio {ratio:.5f}, largest distance {dist:.5f} voxel")
    assert abs(ratio - 1.0) <= 1.25 * 0.01630 and dist <= 1.25 * 0.40666


def test_two_runs_are_equal():
    _, a = _sphere_gpu()
    _, b = _sphere_gpu()
    for k in ("vertices", "colors", "faces"):
        assert torch.equal(a[k], b[k])


# ---------------------------------------------------------------------------------------------------------------- errors
def test_invalid_arguments():
    pts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], device="cuda")
    for voxel in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="voxel must be positive"):
            mesh.TsdfVolume(pts, voxel)
    for trunc in (0.09, 0.81):                                    # T outside [s, 8 s]
        with pytest.raises(ValueError, match="trunc must lie in"):
            mesh.TsdfVolume(pts, 0.1, trunc)
    far = torch.tensor([[0.0, 0.0, 0.0], [1e5, 1e5, 1e5]], device="cuda")
    with pytest.raises(ValueError, match="raise --mesh_voxel"):   # 1251^3 blocks of side 80
        mesh.TsdfVolume(far, 10.0)
    with pytest.raises(ValueError, match="raise --mesh_voxel"):
        mesh.TsdfVolume(far, 1e-9)
    with pytest.raises(ValueError):
        mesh.TsdfVolume(torch.tensor([[0.0, float("inf"), 0.0]], device="cuda"), 1.0)
    with pytest.raises(RuntimeError):
        mesh.TsdfVolume(pts.cpu(), 0.1)
    t = mesh.TsdfVolume(pts, 0.1)
    d, m, im, cam = (torch.ones(2, 4, 5, device="cuda"), torch.ones(2, 4, 5, device="cuda"),
                     torch.zeros(2, 4, 5, 3, dtype=torch.uint8, device="cuda"), torch.eye(4).repeat(2, 2, 1, 1))
    with pytest.raises(ValueError):
        t.integrate(d, m[:1], im, cam)
    with pytest.raises(ValueError):
        t.integrate(d, m, im.float(), cam)
    with pytest.raises(ValueError):
        t.integrate(d, m, im, cam, chunk=33)
    with pytest.raises(RuntimeError):
        t.integrate(d.cpu(), m, im, cam)
    # the C entry points refuse what the wrappers never send
    lib = _lib.load()
    tab = torch.zeros((2, 24), dtype=torch.float64, device="cuda")
    base = [t.keys.data_ptr(), t.n_blocks, t._frame.data_ptr(), t._dims.data_ptr()]
    rest = [d.data_ptr(), m.to(torch.uint8).data_ptr(), im.data_ptr(), tab.data_ptr()]
    acc = [t.sum.data_ptr(), t.n.data_ptr(), t.nc.data_ptr(), t.rgb.data_ptr(), None]
    assert lib.cds_tsdf_integrate_f32(*base, 0.05, *rest, 2, 4, 5, *acc) == _lib.EINVAL          # T < s
    assert lib.cds_tsdf_integrate_f32(*base, 0.9, *rest, 2, 4, 5, *acc) == _lib.EINVAL           # T > 8 s
    assert lib.cds_tsdf_integrate_f32(*base, 0.4, *rest, 33, 4, 5, *acc) == _lib.EINVAL          # more views than a chunk holds
    assert lib.cds_tsdf_integrate_f32(*base, 0.4, *rest, 2, 0, 5, *acc) == _lib.EINVAL
    assert lib.cds_tsdf_integrate_f32(*base, 0.4, rest[0], None, *rest[2:], 2, 4, 5, *acc) == _lib.EINVAL
    bad_dims = torch.tensor([1 << 13, 1 << 13, 2], dtype=torch.int32)                             # 2^27 cells
    assert lib.cds_tsdf_integrate_f32(base[0], base[1], base[2], bad_dims.data_ptr(), 0.4, *rest, 2, 4, 5, *acc) == _lib.EINVAL
    assert lib.cds_tsdf_classify(t.keys.data_ptr(), t.table.data_ptr(), t.n_blocks, t._frame.data_ptr(), t._dims.data_ptr(),
                                 t.sum.data_ptr(), t.n.data_ptr(), 0, None, None, None, None, None) == _lib.EINVAL
    assert float(t.sum.abs().sum()) == 0.0 and int(t.n.sum()) == 0


def test_no_points_gives_the_empty_mesh():
    t = mesh.TsdfVolume(torch.zeros((0, 3), device="cuda"), 0.5)
    assert t.n_blocks == 0
    t.integrate(torch.ones(1, 4, 5, device="cuda"), torch.ones(1, 4, 5, device="cuda"),
                torch.zeros(1, 4, 5, 3, dtype=torch.uint8, device="cuda"), torch.eye(4).repeat(1, 2, 1, 1))
    out = t.extract(2)
    assert out["vertices"].shape == (0, 3) and out["colors"].dtype == torch.uint8 and out["faces"].shape == (0, 3)
    mesh_, vol = mesh.mesh_views([], 0.5)
    assert mesh_["faces"].shape == (0, 3) and vol.n_blocks == 0


# --------------------------------------------------------------------------------------------------------------- harness
VOXEL = 20.0            # a pixel of the 24 x 40 views covers about 18 world units at the surface


def _write_outputs(tmp_path):
    """synth.make_fusion_scene(3, 24, 40) in the layout infer writes: <out>/scan1/{depth_est,confidence,cams,images}."""
    from PIL import Image
    n = 3
    sc = synth.make_fusion_scene(n, 24, 40)
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


def _check_file(path):
    v, c, f = mesh.read_mesh_ply(path)
    assert v.shape == c.shape and np.isfinite(v).all()
    assert f.size == 0 or (f.min() >= 0 and f.max() < len(v))
    assert np.array_equal(pointcloud.read_ply_points(path), v)
    return v, c, f


def _child(module, argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", module] + argv, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout


def test_mesh_scan_and_command_line(tmp_path):
    """Saved depth maps of synth.make_fusion_scene(3, 24, 40): mesh_scan, mesh.main and the command line as a child process write
    the same bytes; the cloud written beside the mesh is the file filter_depth writes alone; an all-masked scan gives the empty
    mesh."""
    scan, pairs = _write_outputs(tmp_path)
    out = tmp_path / "out"
    kw = dict(thres_view=1)
    plain = str(tmp_path / "plain.ply")
    info0 = fusion.filter_depth(str(pairs), str(scan), plain, **kw)
    direct = str(tmp_path / "direct_mesh.ply")
    info = mesh.mesh_scan(str(pairs), str(scan), direct, VOXEL, cloud_ply=str(tmp_path / "beside.ply"), **kw)
    v, c, f = _check_file(direct)
    print(f"{info0['points']} points -> {mesh.format_mesh(info)}")
    assert info["vertices"] == len(v) > 0 and info["faces"] == len(f) > 0 and info["blocks"] > 0
    assert info["cloud"] == info0 and open(tmp_path / "beside.ply", "rb").read() == open(plain, "rb").read()
    tp = M.topology(f, len(v))
    assert tp["edge_uses"].max() <= 2 and tp["directed_unique"]                                 # a manifold with a boundary
    # the mesh lies on the surface the views saw: a vertex is within T = 4 voxels of some view's depth, a depth is at most 6 % of
    # 700 off the height field (the scene's outliers), and a lattice edge is at most sqrt(3) voxels long
    assert np.abs(v[:, 2] - synth.fusion_surface(v[:, 0], v[:, 1])).max() < 4.0 * VOXEL + 0.06 * 700.0 + np.sqrt(3.0) * VOXEL
    # without a cloud: the same mesh
    again = str(tmp_path / "again_mesh.ply")
    assert mesh.mesh_scan(str(pairs), str(scan), again, VOXEL, **kw)["cloud"]["points"] == info0["points"]
    assert open(again, "rb").read() == open(direct, "rb").read()
    cli = ["--testpath", str(tmp_path / "in"), "--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--thres_view", "1",
           "--mesh_voxel", str(VOXEL)]
    assert mesh.main(cli)["scan1"]["vertices"] == len(v)
    assert open(out / "scan1_mesh.ply", "rb").read() == open(direct, "rb").read()
    os.remove(out / "scan1_mesh.ply")
    stdout = _child("cds_mvsnet_amd.mesh", cli)
    assert f"scan1_mesh.ply: {len(v)} vertices, {len(f)} faces, {info['blocks']} blocks" in stdout
    assert open(out / "scan1_mesh.ply", "rb").read() == open(direct, "rb").read()
    # other parameters give other meshes; the dynamic check is accepted
    other = mesh.mesh_scan(str(pairs), str(scan), str(tmp_path / "t_mesh.ply"), VOXEL, trunc=2.0 * VOXEL, min_weight=1, **kw)
    _check_file(str(tmp_path / "t_mesh.ply"))
    assert other["vertices"] > 0 and open(tmp_path / "t_mesh.ply", "rb").read() != open(direct, "rb").read()
    dyn = mesh.mesh_scan(str(pairs), str(scan), str(tmp_path / "d_mesh.ply"), VOXEL, method="dynamic", n_views=(1, 10))
    _check_file(str(tmp_path / "d_mesh.ply"))
    assert "admitted_at" in dyn["cloud"]
    # nothing passes a confidence threshold above 1: no points, no blocks, a valid empty file
    empty = mesh.mesh_scan(str(pairs), str(scan), str(tmp_path / "e_mesh.ply"), VOXEL, conf=(1.5, 1.5, 1.5), **kw)
    assert (empty["vertices"], empty["faces"], empty["blocks"], empty["cloud"]["points"]) == (0, 0, 0, 0)
    ve, ce, fe = _check_file(str(tmp_path / "e_mesh.ply"))
    assert ve.shape == (0, 3) and fe.shape == (0, 3)
    # errors that need the scan
    with pytest.raises(ValueError, match="raise --mesh_voxel"):
        mesh.mesh_scan(str(pairs), str(scan), str(tmp_path / "x_mesh.ply"), 1e-4, **kw)
    with pytest.raises(ValueError, match="gipuma"):
        mesh.mesh_scan(str(pairs), str(scan), str(tmp_path / "x_mesh.ply"), VOXEL, method="gipuma")
    assert not (tmp_path / "x_mesh.ply").exists()


def test_infer_fuse_mesh(tmp_path, capsys):
    """infer --fuse --mesh_voxel on a scene of test_mvs_io._write_scene (3 views of 128 x 160, the smallest the network takes; an
    untrained network, so loose consistency settings): cloud and mesh from one pass.  The mesh equals what mesh_scan and the command
    line make of the depth maps infer saved, and the cloud equals the file of a fusion without --mesh_voxel."""
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanA", 3, 128, 160, seed=3)
    with open(tmp_path / "list.txt", "w") as f:
        f.write("scanA\n")
    out = str(tmp_path / "out")
    fuse = ["--filter_method", "dynamic", "--conf", "0.0,0.0,0.0", "--dyn_dist_base", "2.0", "--dyn_rel_base", "0.02", "--dyn_views",
            "1,10"]
    infer.main(["--testpath", root, "--testlist", str(tmp_path / "list.txt"), "--outdir", out, "--num_view", "3", "--max_h", "128",
                "--max_w", "160", "--interval_scale", "1.0", "--fuse", "--mesh_voxel", "10"] + fuse)
    lines = capsys.readouterr().out.splitlines()
    v, c, f = _check_file(os.path.join(out, "scanA_mesh.ply"))
    line = [ln for ln in lines if "scanA_mesh.ply" in ln]
    assert line and f"{len(v)} vertices, {len(f)} faces" in line[0] and "blocks" in line[0]
    assert [ln for ln in lines if "scanA.ply" in ln and "(dynamic)" in ln]
    via_infer = open(os.path.join(out, "scanA_mesh.ply"), "rb").read()
    cloud = open(os.path.join(out, "scanA.ply"), "rb").read()
    kw = dict(method="dynamic", conf=(0.0, 0.0, 0.0), dist_base=2.0, rel_base=0.02, n_views=(1, 10))
    direct = str(tmp_path / "direct_mesh.ply")
    mesh.mesh_scan(os.path.join(root, "scanA"), os.path.join(out, "scanA"), direct, 10.0, **kw)
    assert open(direct, "rb").read() == via_infer
    os.remove(os.path.join(out, "scanA_mesh.ply"))
    os.remove(os.path.join(out, "scanA.ply"))
    cli = ["--testpath", root, "--outdir", out, "--testlist", str(tmp_path / "list.txt")] + fuse
    _child("cds_mvsnet_amd.mesh", cli + ["--mesh_voxel", "10"])
    assert open(os.path.join(out, "scanA_mesh.ply"), "rb").read() == via_infer
    assert not os.path.exists(os.path.join(out, "scanA.ply"))
    fusion.main(cli)                                               # the fusion alone, without --mesh_voxel
    assert open(os.path.join(out, "scanA.ply"), "rb").read() == cloud
