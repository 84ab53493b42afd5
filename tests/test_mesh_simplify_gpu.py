"""The kernels of csrc/mesh_simplify.hip against the numpy restatement of their rule (mesh_simplify_ref.py): faces,
colours, the info, the fallback flags and the "mean" positions exactly, the "quadric" positions within one fp32 ulp (bit equality
is expected; the bar only admits a tie of the double rounding fp64 -> fp32).  Then the way to a simplified mesh file through
mesh_scan, the command line, --from_mesh and infer --fuse --mesh_voxel --render_mesh."""
import filecmp
import functools
import os

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_ref as M
import mesh_simplify_ref as R
from cds_mvsnet_amd import _lib, infer, mesh, mvs_io, render
from cds_mvsnet_amd.pointcloud import unpack_colors, voxel_groups
from test_mesh_gpu import VOXEL, _check_file, _child, _write_outputs
from test_mvs_io import _write_scene
from test_render_gpu import FUSE, _tree

pytestmark = pytest.mark.gpu

SEEN = {"positions": 0, "off_by_one_ulp": 0}       # quadric coordinates compared in this run, and those not bit-equal


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}, expected {want.dtype} {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what} differs"


def _close(got, want, what):
    """Quadric positions: at most one fp32 ulp apart."""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}"
    assert np.isfinite(got).all()
    SEEN["positions"] += got.size
    SEEN["off_by_one_ulp"] += int((got.view(np.uint32) != want.view(np.uint32)).sum())
    d = R.ulp_distance(got, want)
    print(f"{what}: {d} ulp at most; quadric coordinates compared so far {SEEN['positions']}, not bit-equal {SEEN['off_by_one_ulp']}")
    assert d <= 1, f"{what}: {d} ulp apart"


def _upload(v, c, f):
    return {"vertices": torch.from_numpy(np.ascontiguousarray(v)).cuda(), "colors": torch.from_numpy(np.ascontiguousarray(c)).cuda(),
            "faces": torch.from_numpy(np.ascontiguousarray(f)).cuda()}


@functools.lru_cache(maxsize=None)
def _want(name, cell, placement):
    """The restatement's result for a named mesh; computed once per (mesh, cell, placement), not to be modified."""
    return R.simplify(*MESHES[name](), cell, placement)


def _sphere():
    m = M.analytic_case("sphere")[1]
    return m["vertices"], m["colors"], m["faces"]


def _random():
    rng = np.random.default_rng(4)
    return rng.uniform(0, 6, (500, 3)).astype(np.float32), R.colors_for(500, 3), C.random_faces(500, 2000, seed=2)


def _sparse():
    v, c, f = C.isolated_triangles(70, n_vertices=100003, seed=7)
    return (v * np.float32(3.0)).astype(np.float32), c, f


MESHES = {"sphere": _sphere, "debris": C.sphere_with_debris, "cube": R.cube, "plate": R.plate, "fan": R.fan_and_triangles,
          "plane": lambda: R.tilted_plane()[:3], "cone_near": lambda: R.cone_band(0.6, 0.4)[:3],
          "cone_far": lambda: R.cone_band(3.0, 0.1)[:3], "random": _random, "sparse": _sparse}


def _check(v, c, f, cell, placement, want, what):
    """simplify_mesh and the per-cluster results of its kernels on the device against the restatement -> (mesh as numpy, info)."""
    wout, winfo, detail = want
    m = _upload(v, c, f)
    got, info = mesh.simplify_mesh(m, cell, placement)
    out = {}
    for k in ("vertices", "colors", "faces"):
        assert got[k].is_cuda and got[k].is_contiguous()
        out[k] = got[k].cpu().numpy()
    _same(out["faces"], wout["faces"], f"{what}: faces")
    _same(out["colors"], wout["colors"], f"{what}: colors")
    (_same if placement == "mean" else _close)(out["vertices"], wout["vertices"], f"{what}: vertices")
    assert info == winfo, f"{what}: {info}, expected {winfo}"
    if detail is not None:                                               # every cluster, kept or not
        nc, pos, packed, fell, fclus, gone, ident = mesh._clusters(m["vertices"], m["colors"], m["faces"], float(cell), placement)
        assert nc == winfo["clusters"]
        (_same if placement == "mean" else _close)(pos.cpu().numpy(), detail["positions"], f"{what}: cluster positions")
        _same(unpack_colors(packed).cpu().numpy(), detail["colors"], f"{what}: cluster colours")
        if placement == "quadric":
            _same(fell.cpu().numpy(), detail["fallback"].astype(np.uint8), f"{what}: fallback flags")
        else:
            assert fell is None
        _same(gone.cpu().numpy(), detail["collapsed"].astype(np.uint8), f"{what}: collapsed flags")
        _same(fclus.cpu().numpy(), detail["cluster"][f].astype(np.int32), f"{what}: face clusters")
    return out, info


def _named(name, cell, placement):
    return _check(*MESHES[name](), cell, placement, _want(name, cell, placement), f"{name}, cell {cell}, {placement}")


# ---------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("placement", ["quadric", "mean"])
@pytest.mark.parametrize("cell", [0.25, 1.0, 2.0, 3.0])
def test_sphere(cell, placement):
    out, info = _named("sphere", cell, placement)
    assert R.closed(out["faces"]) and info["fallback"] == 0
    if cell == 2.0:
        assert info["vertices"] == (2286, 163) and info["faces"] == (4568, 330)


@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_sphere_one_cluster_and_debris(placement):
    out, info = _named("sphere", 100.0, placement)
    assert info["clusters"] == 1 and out["faces"].shape == (0, 3) and out["vertices"].shape == (0, 3)
    out, info = _named("debris", 2.0, placement)
    assert info["clusters"] == 167 and info["vertices"] == (2294, 163)


@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_cube_plane_plate(placement):
    out, info = _named("cube", 1.0, placement)
    assert info["vertices"] == (1538, 98) and info["faces"] == (3072, 192)
    volume = M.signed_volume(out["vertices"], out["faces"])
    assert volume > 63.9 if placement == "quadric" else volume < 60.0
    _named("plane", 1.0, placement)
    out, info = _named("plate", 1.0, placement)
    assert info["duplicates"] == 0 and info["faces"][1] > 0


def test_cone_pair():
    out, info = _named("cone_near", 1.0, "quadric")
    assert info["fallback"] == 0
    out, info = _named("cone_far", 1.0, "quadric")
    assert info["fallback"] == 1
    _named("cone_far", 1.0, "mean")
    vz = np.array([[5.0, 5.0, 5.0], [5.1, 5.1, 5.1], [5.2, 5.2, 5.2], [0.0, 0.0, 0.0]], np.float32)       # zero areas only
    fz = np.array([[0, 1, 2], [3, 3, 0]], np.int32)
    cz = R.colors_for(4, 1)
    out, info = _check(vz, cz, fz, 1.0, "quadric", R.simplify(vz, cz, fz, 1.0), "zero area")
    assert info["fallback"] == 2


@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, 1000])
def test_isolated_triangles(n_faces):
    """Around the launch shapes; normal positions (sigma 1) and a cell of 1.5 put several vertices in a cluster."""
    v, c, f = C.isolated_triangles(n_faces, seed=n_faces)
    for placement in ("quadric", "mean"):
        out, info = _check(v, c, f, 1.5, placement, R.simplify(v, c, f, 1.5, placement), f"{n_faces} triangles, {placement}")
        assert info["clusters"] < len(v) or n_faces == 1
    if n_faces == 1000:
        assert info["collapsed"] > 0 and info["faces"][1] > 0


@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_random_faces(placement):
    out, info = _named("random", 1.5, placement)
    assert info["collapsed"] > 0 and info["duplicates"] > 0 and info["faces"][1] > 0


def test_duplicates_by_three_sorts(monkeypatch):
    """The identities of more clusters than a packed key holds go through one stable sort per column: the same faces stay."""
    v, c, f = _random()
    want = _want("random", 1.5, "mean")
    monkeypatch.setattr(mesh, "PACK_BITS", 3)                            # 8 < the 64 clusters of this mesh
    assert want[1]["clusters"] > 8
    _check(v, c, f, 1.5, "mean", want, "three sorts")


def test_fan_in_one_cell_next_to_small_clusters():
    """One cluster with thousands of incidences, a long serial chain, among clusters of a few."""
    want = _want("fan", 1.0, "quadric")
    inc = want[2]["incidences"]
    assert inc.max() > 5000 and np.median(inc) < 10
    _named("fan", 1.0, "quadric")
    _named("fan", 1.0, "mean")


def test_many_more_vertices_than_referenced():
    out, info = _named("sparse", 1.0, "quadric")
    assert info["vertices"][0] == 100003 and info["clusters"] > info["vertices"][1]
    _named("sparse", 1.0, "mean")


def test_empty_meshes_make_no_launch(monkeypatch):
    def no_launch():
        raise AssertionError("the library was loaded: a launch was about to happen")
    monkeypatch.setattr(mesh._lib, "load", no_launch)
    f0 = np.zeros((0, 3), np.int32)
    for nv in (0, 5):
        v, c = np.zeros((nv, 3), np.float32), np.zeros((nv, 3), np.uint8)
        for placement in ("quadric", "mean"):
            out, info = _check(v, c, f0, 1.0, placement, R.simplify(v, c, f0, 1.0, placement), f"F = 0, V = {nv}")
            assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3) and info["vertices"] == (nv, 0)


def test_two_runs_are_equal():
    m = _upload(*R.fan_and_triangles())
    for placement in ("quadric", "mean"):
        (a, ia), (b, ib) = mesh.simplify_mesh(m, 1.0, placement), mesh.simplify_mesh(m, 1.0, placement)
        assert ia == ib and all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def test_errors():
    v, c, f = R.cube()
    m = _upload(v, c, f)
    for k in ("vertices", "colors", "faces"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mesh.simplify_mesh(dict(m, **{k: m[k].cpu()}), 1.0)
    for bad in (np.array([[0, 1, len(v)]], np.int32), np.array([[0, -1, 2]], np.int32)):
        with pytest.raises(ValueError, match="outside the 1538 vertices"):
            mesh.simplify_mesh(dict(m, faces=torch.from_numpy(bad).cuda()), 1.0)
    for bad in (m["faces"].long(), m["faces"][:, :2], m["faces"].reshape(-1)):
        with pytest.raises(ValueError, match="faces must be an int32"):
            mesh.simplify_mesh(dict(m, faces=bad), 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell must be positive"):
            mesh.simplify_mesh(m, bad)
    with pytest.raises(ValueError, match="placement"):
        mesh.simplify_mesh(m, 1.0, "median")
    for bad in (float("nan"), float("inf")):
        vb = m["vertices"].clone()
        vb[77, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            mesh.simplify_mesh(dict(m, vertices=vb), 1.0)
    with pytest.raises(ValueError, match="voxels along one axis"):
        mesh.simplify_mesh(m, 1e-7)


def test_entry_points_skip_what_the_wrapper_never_sends():
    """A face with an index outside the vertices is written as collapsed and skipped by the sums: the positions, flags and marks are
    those of the mesh without it.  Null pointers and sizes out of range are CDS_EINVAL."""
    lib = _lib.load()
    v, c, good = _random()
    nv = len(v)
    bad = np.insert(good, [0, 700, 700, 2000], np.array([[0, 1, nv], [-1, 0, 4], [3, 2 ** 31 - 1, 5], [nv + 7, 2, 3]], np.int32), axis=0)
    valid = np.ones(len(bad), bool)
    valid[[0, 701, 702, 2003]] = False
    assert np.array_equal(bad[valid], good)
    tv = torch.from_numpy(v).cuda()
    perm, start, ukeys, counts = voxel_groups(tv, 1.5)
    nc = int(ukeys.numel())
    cluster = torch.empty(nv, dtype=torch.int32, device="cuda")
    cluster[perm] = torch.repeat_interleave(torch.arange(nc, dtype=torch.int32, device="cuda"), counts)
    res = {}
    for name, faces in (("good", good), ("bad", bad)):
        tf, nf = torch.from_numpy(faces).cuda(), len(faces)
        fclus = torch.full((nf, 3), 9, dtype=torch.int32, device="cuda")
        ident = torch.full((nf, 3), 9, dtype=torch.int32, device="cuda")
        gone = torch.full((nf,), 7, dtype=torch.uint8, device="cuda")
        assert lib.cds_mesh_simplify_faces(tf.data_ptr(), nf, nv, cluster.data_ptr(), nc, fclus.data_ptr(), gone.data_ptr(),
                                           ident.data_ptr(), None) == 0
        owner, inc = torch.sort(fclus.reshape(-1), stable=True)
        inc_start = torch.searchsorted(owner, torch.arange(nc + 1, dtype=torch.int32, device="cuda")).to(torch.int32)
        pos = torch.empty((nc, 3), dtype=torch.float32, device="cuda")
        fell = torch.empty(nc, dtype=torch.uint8, device="cuda")
        assert lib.cds_mesh_simplify_quadric_f32(tv.data_ptr(), nv, tf.data_ptr(), nf, perm.data_ptr(), start.data_ptr(), inc.data_ptr(),
                                                 inc_start.data_ptr(), nc, 1.5, pos.data_ptr(), fell.data_ptr(), None) == 0
        fkeep = torch.ones(nf, dtype=torch.uint8, device="cuda")         # even the faces outside: mark and gather skip them
        ckeep = torch.zeros(nc, dtype=torch.uint8, device="cuda")
        assert lib.cds_mesh_simplify_mark(fclus.data_ptr(), fkeep.data_ptr(), nf, nc, ckeep.data_ptr(), None) == 0
        cnew = (torch.cumsum(ckeep, 0, dtype=torch.int64) - ckeep).to(torch.int32)
        fnew = torch.arange(nf, dtype=torch.int32, device="cuda")
        n_out = int(ckeep.sum())
        vout = torch.zeros((n_out, 3), dtype=torch.float32, device="cuda")
        fout = torch.full((nf, 3), -5, dtype=torch.int32, device="cuda")
        assert lib.cds_mesh_simplify_gather(pos.data_ptr(), None, nc, ckeep.data_ptr(), cnew.data_ptr(), fclus.data_ptr(), nf,
                                            fkeep.data_ptr(), fnew.data_ptr(), n_out, nf, vout.data_ptr(), None, fout.data_ptr(), None) == 0
        torch.cuda.synchronize()
        res[name] = tuple(t.cpu().numpy() for t in (fclus, ident, gone, pos, fell, ckeep, vout, fout))
    g, b = res["good"], res["bad"]
    for k, what in ((0, "face clusters"), (1, "identities"), (2, "collapsed"), (7, "gathered faces")):
        _same(b[k][valid], g[k], what)
    assert (b[0][~valid] == -1).all() and (b[1][~valid] == -1).all() and (b[2][~valid] == 1).all() and (b[7][~valid] == -5).all()
    for k, what in ((3, "positions"), (4, "fallback"), (5, "marks"), (6, "gathered positions")):
        _same(b[k], g[k], what)
    detail = _want("random", 1.5, "quadric")[2]
    _close(g[3], detail["positions"], "positions through the entry points")
    p = torch.zeros(64, dtype=torch.int64, device="cuda").data_ptr()
    E = _lib.EINVAL
    assert lib.cds_mesh_simplify_faces(None, 1, 8, p, 2, p, p, p, None) == E and lib.cds_mesh_simplify_faces(p, 1, 8, p, 2, p, None, p, None) == E
    assert lib.cds_mesh_simplify_faces(p, 1, 8, None, 2, p, p, p, None) == E and lib.cds_mesh_simplify_faces(p, 2 ** 31, 8, p, 2, p, p, p, None) == E
    assert lib.cds_mesh_simplify_faces(p, 1, 8, p, 9, p, p, p, None) == E and lib.cds_mesh_simplify_faces(p, -1, 8, p, 2, p, p, p, None) == E
    assert lib.cds_mesh_simplify_faces(None, 0, 8, None, 2, None, None, None, None) == 0
    q = lib.cds_mesh_simplify_quadric_f32
    assert q(None, 8, p, 1, p, p, p, p, 2, 1.0, p, p, None) == E and q(p, 8, None, 1, p, p, p, p, 2, 1.0, p, p, None) == E
    assert q(p, 8, p, 1, p, p, p, p, 2, 0.0, p, p, None) == E and q(p, 8, p, 1, p, p, p, p, 2, float("nan"), p, p, None) == E
    assert q(p, 8, p, 1, p, p, p, p, 2, float("inf"), p, p, None) == E and q(p, 8, p, 1, p, p, p, p, 9, 1.0, p, p, None) == E
    assert q(p, 8, p, 2 ** 31 // 3 + 1, p, p, p, p, 2, 1.0, p, p, None) == E and q(p, 8, p, 1, p, p, p, p, 2, 1.0, p, None, None) == E
    assert q(None, 8, None, 1, None, None, None, None, 0, 1.0, None, None, None) == 0
    assert lib.cds_mesh_simplify_mark(None, p, 1, 2, p, None) == E and lib.cds_mesh_simplify_mark(p, p, 1, 2, None, None) == E
    assert lib.cds_mesh_simplify_mark(p, p, 1, 2 ** 31, p, None) == E and lib.cds_mesh_simplify_mark(None, None, 0, 2, None, None) == 0
    ga = lib.cds_mesh_simplify_gather
    assert ga(p, None, 2, p, p, p, 1, p, p, 3, 1, p, None, p, None) == E                           # more out than in
    assert ga(p, None, 2, p, p, p, 1, p, p, 2, 2, p, None, p, None) == E
    assert ga(None, None, 2, p, p, p, 1, p, p, 2, 1, p, None, p, None) == E
    assert ga(p, p, 2, p, p, p, 1, p, p, 2, 1, p, None, p, None) == E                              # colours in, nowhere to put them
    assert ga(p, None, 2, p, p, None, 1, p, p, 2, 1, p, None, p, None) == E
    assert ga(None, None, 2, None, None, None, 1, None, None, 0, 0, None, None, None, None) == 0
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------------- end to end
def _same_file(path, want, placement, what):
    """A written mesh against the restatement's arrays: faces and colours exactly, positions as the placement's bar says."""
    v, c, f = _check_file(path)
    _same(f, want["faces"], f"{what}: faces")
    _same(c, want["colors"], f"{what}: colors")
    (_same if placement == "mean" else _close)(v, want["vertices"], f"{what}: vertices")
    return v, c, f


def test_mesh_scan_and_command_line(tmp_path, capsys, monkeypatch):
    """The synthetic scan of test_mesh_gpu (3 views of 24 x 40): the file written with a cell is simplify_mesh of the file written
    without one, through mesh_scan, mesh.main and a child process; without the option no byte changes and nothing of this runs;
    --from_mesh simplifies a saved file, after its clean-up when both are asked."""
    scan, pairs = _write_outputs(tmp_path)
    out = tmp_path / "out"
    kw = dict(thres_view=1)
    plain = str(tmp_path / "plain_mesh.ply")
    info0 = mesh.mesh_scan(str(pairs), str(scan), plain, VOXEL, **kw)
    arrays = mesh.read_mesh_ply(plain)
    assert len(arrays[2]) > 0
    def no_simplify(*a, **k):
        raise AssertionError("simplify_mesh ran without a cell")
    zero = str(tmp_path / "zero_mesh.ply")
    with monkeypatch.context() as mp:
        mp.setattr(mesh, "simplify_mesh", no_simplify)
        info = mesh.mesh_scan(str(pairs), str(scan), zero, VOXEL, simplify=0.0, **kw)
        cli = ["--testpath", str(tmp_path / "in"), "--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--thres_view", "1",
               "--mesh_voxel", str(VOXEL)]
        mesh.main(cli)
    assert filecmp.cmp(plain, zero, shallow=False) and sorted(info) == sorted(info0) == ["blocks", "cloud", "faces", "mesh", "vertices"]
    assert open(out / "scan1_mesh.ply", "rb").read() == open(plain, "rb").read()
    cell = 2.0 * VOXEL
    want = {p: R.simplify(*arrays, cell, p) for p in ("quadric", "mean")}
    assert 0 < want["quadric"][1]["faces"][1] < len(arrays[2])
    for placement in ("quadric", "mean"):
        direct = str(tmp_path / f"direct_{placement}_mesh.ply")
        info = mesh.mesh_scan(str(pairs), str(scan), direct, VOXEL, simplify=cell, placement=placement, **kw)
        _same_file(direct, want[placement][0], placement, f"mesh_scan, {placement}")
        assert info["simplify"] == want[placement][1] and info["faces"] == want[placement][1]["faces"][1] and "clean" not in info
        assert info["blocks"] == info0["blocks"]
        assert torch.equal(info["mesh"]["faces"].cpu(), torch.from_numpy(mesh.read_mesh_ply(direct)[2]))     # what render_scan gets
        assert np.array_equal(info["mesh"]["vertices"].cpu().numpy().view(np.uint32), mesh.read_mesh_ply(direct)[0].view(np.uint32))
    capsys.readouterr()
    res = mesh.main(cli + ["--mesh_simplify", str(cell)])
    line = capsys.readouterr().out
    w = want["quadric"][1]
    assert res["scan1"]["simplify"] == w and f"simplified {w['vertices'][0]} -> {w['vertices'][1]} vertices" in line
    assert f"{w['collapsed']} faces collapsed, {w['duplicates']} duplicates, {w['fallback']} fallbacks" in line
    _same_file(str(out / "scan1_mesh.ply"), want["quadric"][0], "quadric", "mesh.main")
    os.remove(out / "scan1_mesh.ply")
    stdout = _child("cds_mvsnet_amd.mesh", cli + ["--mesh_simplify", str(cell), "--mesh_simplify_placement", "mean"])
    _same_file(str(out / "scan1_mesh.ply"), want["mean"][0], "mean", "child process")
    assert "scan1_mesh.ply:" in stdout and "simplified" in stdout
    # --from_mesh: the saved plain mesh with debris appended, simplified alone, then cleaned and simplified
    v, c, f = arrays
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    v2 = np.concatenate([v, v.max(0) + 30 * VOXEL + corner]).astype(np.float32)
    c2 = np.concatenate([c, np.full((4, 3), 200, np.uint8)])
    f2 = np.concatenate([f, C.TETRA + len(v)]).astype(np.int32)
    saved = str(tmp_path / "saved_mesh.ply")
    mesh.write_mesh_ply(saved, v2, c2, f2)
    base = ["--from_mesh", saved, "--outdir", str(out), "--testlist", str(tmp_path / "list.txt")]
    res = mesh.main(base + ["--mesh_simplify", str(cell)])
    wout, winfo, _ = R.simplify(v2, c2, f2, cell)
    _same_file(str(out / "scan1_mesh.ply"), wout, "quadric", "--from_mesh")
    assert res["scan1"]["simplify"] == winfo and "clean" not in res["scan1"] and winfo["clusters"] > winfo["vertices"][1]
    res = mesh.main(base + ["--mesh_simplify", str(cell), "--mesh_min_component", "5", "--mesh_simplify_placement", "mean"])
    cleaned, cinfo = C.clean(v2, c2, f2, min_faces=5)
    wout, winfo, _ = R.simplify(cleaned["vertices"], cleaned["colors"], cleaned["faces"], cell, "mean")
    _same_file(str(out / "scan1_mesh.ply"), wout, "mean", "--from_mesh, cleaned first")
    assert res["scan1"]["clean"]["faces"] == cinfo["faces"] and res["scan1"]["simplify"] == winfo
    assert "blocks" not in capsys.readouterr().out
    assert open(saved, "rb").read() and mesh.read_mesh_ply(saved)[2].shape == f2.shape             # the source is not touched


@pytest.fixture(scope="module")
def plain_infer(tmp_path_factory):
    """infer --fuse --mesh_voxel 10 without the new options on a scene of test_mvs_io._write_scene (3 views of 128 x 160, an
    untrained network, the loose settings of test_mesh_gpu.test_infer_fuse_mesh) -> (root, list, base arguments, output folder)."""
    tmp = tmp_path_factory.mktemp("simplify_infer")
    root = str(tmp / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanA", 3, 128, 160, seed=3)
    lst = str(tmp / "list.txt")
    with open(lst, "w") as f:
        f.write("scanA\n")
    base = ["--testpath", root, "--testlist", lst, "--num_view", "3", "--max_h", "128", "--max_w", "160", "--interval_scale", "1.0",
            "--fuse", "--mesh_voxel", "10"] + FUSE
    plain = str(tmp / "plain")
    def no_simplify(*a, **k):
        raise AssertionError("simplify_mesh ran without --mesh_simplify")
    with pytest.MonkeyPatch.context() as mp:                             # without the option nothing of this runs
        mp.setattr(mesh, "simplify_mesh", no_simplify)
        infer.main(base + ["--outdir", plain])
    return tmp, root, base, plain


def test_infer_simplify_and_render(plain_infer, capsys):
    """infer --fuse --mesh_voxel --mesh_simplify CELL --render_mesh: the mesh file is simplify_mesh of the file of the run without
    the option (in which simplify_mesh is not called), every other file is that run's, and depth_mesh is render_scan of the
    simplified file."""
    tmp, root, base, plain = plain_infer
    arrays = mesh.read_mesh_ply(os.path.join(plain, "scanA_mesh.ply"))
    cell = 30.0
    wout, winfo, _ = R.simplify(*arrays, cell)
    assert 0 < winfo["faces"][1] < winfo["faces"][0]
    out = str(tmp / "simple")
    capsys.readouterr()
    infer.main(base + ["--outdir", out, "--mesh_simplify", str(cell), "--render_mesh"])
    lines = capsys.readouterr().out.splitlines()
    _same_file(os.path.join(out, "scanA_mesh.ply"), wout, "quadric", "infer")
    line = [ln for ln in lines if "scanA_mesh.ply" in ln]
    assert line and f"{winfo['faces'][1]} faces" in line[0] and f"{winfo['faces'][0]} -> {winfo['faces'][1]} faces" in line[0]
    for name in _tree(plain):
        if name != "scanA_mesh.ply":
            assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    scan = os.path.join(out, "scanA")
    render.render_scan(scan, os.path.join(out, "scanA_mesh.ply"), os.path.join(root, "scanA"), subdir="again")
    render.render_scan(scan, os.path.join(plain, "scanA_mesh.ply"), os.path.join(root, "scanA"), subdir="full")
    differ = 0
    for i in range(3):
        a = mvs_io.read_pfm(os.path.join(scan, "depth_mesh", f"{i:08d}.pfm"))[0]
        b = mvs_io.read_pfm(os.path.join(scan, "again", f"{i:08d}.pfm"))[0]
        d = mvs_io.read_pfm(os.path.join(scan, "full", f"{i:08d}.pfm"))[0]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (a > 0).any()
        differ += int((a.view(np.uint32) != d.view(np.uint32)).sum())
    assert differ > 0                                                    # the maps are those of the simplified mesh
    print(f"cell {cell}: {winfo['faces'][0]} -> {winfo['faces'][1]} faces; {differ} pixels of depth_mesh change")
