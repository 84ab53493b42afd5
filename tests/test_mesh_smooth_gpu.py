"""The kernels of csrc/mesh_smooth.hip against the numpy restatement of their rule (mesh_smooth_ref.py): the
adjacency, the faces, the colours and the info exactly, the positions bit for bit, and within one fp32 ulp for the vertices the
limit moved (the device's sqrt and the double rounding fp64 -> fp32).  Then the way to a smoothed mesh file through mesh_scan, the
command line, --from_mesh and infer --fuse --mesh_voxel --render_mesh."""
import filecmp
import functools
import os

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_ref as M
import mesh_simplify_ref as R
import mesh_smooth_ref as S
import mesh_weighted_ref as W
from cds_mvsnet_amd import _lib, fusion, infer, mesh, mvs_io, render
from test_mesh_gpu import VOXEL, _check_file, _child, _write_outputs
from test_mesh_weighted_gpu import _sphere_records
from test_mvs_io import _write_scene
from test_render_gpu import FUSE, _tree

pytestmark = pytest.mark.gpu

SEEN = {"clamped": 0, "off_by_one_ulp": 0}         # clamped coordinates compared in this run, and those not bit-equal

# name -> (the mesh, a limit for it); the limit of the noisy sphere clamps some of its vertices and not all
CASES = {"sphere": (S.sphere, 0.08), "noisy": (S.noisy_sphere, 0.08), "debris": (C.sphere_with_debris, 0.08),
         "patch": (S.grid_patch, 0.1), "sparse": (S.sparse_triangles, 1.0), "random": (S.random_faces, 1.0),
         "dense": (S.dense_faces, 1.0),         "repeated": (S.repeated_corners, 1.0), "hub": (S.hub_fan, 5.2), "fans": (S.small_fans, 5.0),
         "strip": (S.strip_and_triangles, 1.0)}
# (iterations, lam, mu, limited): every value of every parameter; the noisy sphere takes the full product below
COMBOS = [(1, 0.5, -0.53, False), (7, 0.5, -0.53, False), (7, 1.0, 0.0, False), (7, 0.5, -0.53, True), (1, 1.0, 0.0, True)]
PRODUCT = [(i, l, m, d) for i in (1, 7) for l in (0.5, 1.0) for m in (-0.53, 0.0) for d in (False, True)]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}, expected {want.dtype} {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what} differs"


def _upload(v, c, f):
    return {"vertices": torch.from_numpy(np.ascontiguousarray(v)).cuda(), "colors": torch.from_numpy(np.ascontiguousarray(c)).cuda(),
            "faces": torch.from_numpy(np.ascontiguousarray(f)).cuda()}


@functools.lru_cache(maxsize=None)
def _adj(name):
    """The restatement's adjacency of a named mesh; computed once, not to be modified."""
    v, c, f = CASES[name][0]()
    return S.adjacency(f, len(v))


@functools.lru_cache(maxsize=None)
def _want(name, iterations, lam, mu, max_move):
    v, c, f = CASES[name][0]()
    return S.smooth(v, c, f, iterations, lam, mu, max_move, adj=_adj(name))


def _check_adjacency(got, want, what):
    g = {k: t.cpu().numpy() for k, t in got.items()}
    _same(g["start"], want["start"], f"{what}: start")
    _same(g["degree"], want["degree"], f"{what}: degree")
    _same(g["boundary"], want["boundary"], f"{what}: boundary")
    _same(g["isolated"], want["isolated"], f"{what}: isolated")
    assert g["neighbors"].dtype == np.int32 and g["neighbors"].shape == want["neighbors"].shape
    _same(S.used(g), S.used(want), f"{what}: neighbours")


def _check_positions(got, want, unlimited, v0, max_move, what):
    """Bit for bit, but for the vertices the limit moved: those within one fp32 ulp, counted and printed.  unlimited: the
    restatement's positions without a limit, from which rule 6 says which vertices those are."""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    if max_move == 0:
        return _same(got, want, what)
    free = ~S.limit(v0, unlimited, max_move)[2]
    _same(got[free], want[free], f"{what}: vertices inside the limit")
    if (~free).any():
        SEEN["clamped"] += int((~free).sum()) * 3
        SEEN["off_by_one_ulp"] += int((got[~free].view(np.uint32) != want[~free].view(np.uint32)).sum())
        ulp = R.ulp_distance(got[~free], want[~free])
        print(f"{what}: {ulp} ulp at most over {int((~free).sum())} clamped vertices; clamped coordinates compared so far "
              f"{SEEN['clamped']}, not bit-equal {SEEN['off_by_one_ulp']}")
        assert ulp <= 1, f"{what}: {ulp} ulp apart"


def _run(name, iterations, lam, mu, limited):
    v, c, f = CASES[name][0]()
    max_move = CASES[name][1] if limited else 0.0
    wout, winfo = _want(name, iterations, lam, mu, max_move)
    what = f"{name}, {iterations} iterations, lam {lam}, mu {mu}, max_move {max_move}"
    m = _upload(v, c, f)
    before = {k: t.clone() for k, t in m.items()}
    got, info = mesh.smooth_mesh(m, iterations, lam, mu, max_move)
    assert all(torch.equal(m[k].view(torch.uint8), before[k].view(torch.uint8)) for k in m), f"{what}: the input changed"
    assert got["vertices"].is_cuda and got["vertices"].is_contiguous() and got["vertices"].data_ptr() != m["vertices"].data_ptr()
    _same(got["faces"].cpu().numpy(), f, f"{what}: faces")
    _same(got["colors"].cpu().numpy(), c, f"{what}: colors")
    _check_positions(got["vertices"].cpu().numpy(), wout["vertices"], _want(name, iterations, lam, mu, 0.0)[0]["vertices"], v, max_move,
                     f"{what}: vertices")
    assert info == winfo, f"{what}: {info}, expected {winfo}"
    return got, info


# ---------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", list(CASES))
def test_adjacency(name):
    v, c, f = CASES[name][0]()
    want = _adj(name)
    _check_adjacency(mesh.mesh_adjacency(torch.from_numpy(f).cuda(), len(v)), want, name)
    if name == "hub":
        assert want["degree"][0] == 5000 and np.diff(want["start"])[0] == 10000 > mesh.ADJ_SMALL and not want["boundary"][0]
    if name == "fans":                                                   # segments on either side of the finishing kernel's own sort
        assert np.diff(want["start"])[[0, 63, 128]].tolist() == [mesh.ADJ_SMALL - 2, mesh.ADJ_SMALL, mesh.ADJ_SMALL + 2]
    if name == "dense":                                                  # multiplicities above 2 in segments of both kinds
        assert M.topology(f, len(v))["edge_uses"].max() > 2
        assert np.diff(want["start"]).max() > mesh.ADJ_SMALL > np.diff(want["start"]).min()
    if name == "sparse":
        assert want["isolated"].sum() == 100003 - 210 and want["boundary"].sum() == 210
    if name == "strip":
        assert len(want["degree"]) == (1 << 16) + 30000 > 256 * 300                              # hundreds of workgroups


@pytest.mark.parametrize("iterations, lam, mu, limited", COMBOS)
@pytest.mark.parametrize("name", [n for n in CASES if n != "noisy"])
def test_smooth_vs_restatement(name, iterations, lam, mu, limited):
    got, info = _run(name, iterations, lam, mu, limited)
    if name == "sparse":                                                 # -0.0 and denormals in isolated vertices keep their bits
        v = CASES[name][0]()[0]
        iso = _adj(name)["isolated"]
        _same(got["vertices"].cpu().numpy()[iso], v[iso], "isolated vertices")
        assert (v[iso] == 0).any() and (np.abs(v[iso][v[iso] != 0]) < 1e-38).any() and np.signbit(v[iso]).any()
    if name == "patch":
        assert info["boundary"] == 28 and (got["vertices"][:, 2] == 2.5).all()
    if name == "hub":
        assert info["isolated"] == 0 and info["boundary"] == 10000


@pytest.mark.parametrize("iterations, lam, mu, limited", PRODUCT)
def test_noisy_sphere(iterations, lam, mu, limited):
    got, info = _run("noisy", iterations, lam, mu, limited)
    assert info["boundary"] == 0 and info["isolated"] == 0
    if limited:
        assert 0 < info["clamped"] < info["vertices"]                    # the limit clamps some vertices and not all
    if (iterations, lam, mu, limited) == (7, 0.5, -0.53, False):
        v, c, f = S.noisy_sphere()
        before, after = S.sphere_errors(v, f), S.sphere_errors(got["vertices"].cpu().numpy(), f)
        print(f"noisy sphere, 7 iterations on the device: rms {before[0]:.4f} -> {after[0]:.4f}, normals {before[1]:.2f} -> {after[1]:.2f} deg")
        assert after[0] < 0.5 * before[0] and after[1] < before[1]


def test_two_runs_are_equal():
    """The fill order of the atomics does not show: the segments are sorted sets."""
    for name in ("random", "hub"):
        v, c, f = CASES[name][0]()
        m = _upload(v, c, f)
        (a, ia), (b, ib) = mesh.smooth_mesh(m, 3, max_move=1.0), mesh.smooth_mesh(m, 3, max_move=1.0)
        assert ia == ib and torch.equal(a["vertices"].view(torch.int32), b["vertices"].view(torch.int32))
        x, y = mesh.mesh_adjacency(m["faces"], len(v)), mesh.mesh_adjacency(m["faces"], len(v))
        assert all(torch.equal(x[k], y[k]) for k in ("start", "degree", "boundary", "isolated"))
        assert np.array_equal(S.used({k: t.cpu().numpy() for k, t in x.items()}), S.used({k: t.cpu().numpy() for k, t in y.items()}))


def test_empty_meshes_and_meshes_without_an_edge_make_no_step():
    f0 = np.zeros((0, 3), np.int32)
    for nv, f in ((0, f0), (5, f0), (5, np.array([[2, 2, 2], [4, 4, 4]], np.int32))):
        v, c = C._positions(nv, 1), C._colors(nv, 1)
        m = _upload(v, c, f)
        got, info = mesh.smooth_mesh(m, 4, max_move=0.5)
        want, winfo = S.smooth(v, c, f, 4, max_move=0.5)
        assert info == winfo == {"iterations": 4, "lam": 0.5, "mu": -0.53, "vertices": nv, "boundary": 0, "isolated": nv, "clamped": 0,
                                 "max_move": 0.0}
        assert all(got[k] is m[k] for k in m)                            # the input, unchanged
        adj = mesh.mesh_adjacency(m["faces"], nv)
        _check_adjacency(adj, S.adjacency(f, nv), f"V = {nv}, F = {len(f)}")
        assert adj["isolated"].all() and adj["neighbors"].numel() == 0


def test_errors():
    v, c, f = S.grid_patch()
    m = _upload(v, c, f)
    for k in ("vertices", "colors", "faces"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mesh.smooth_mesh(dict(m, **{k: m[k].cpu()}), 2)
    for bad in (np.array([[0, 1, len(v)]], np.int32), np.array([[0, -1, 2]], np.int32)):
        with pytest.raises(ValueError, match="outside the 63 vertices"):
            mesh.smooth_mesh(dict(m, faces=torch.from_numpy(bad).cuda()), 2)
        with pytest.raises(ValueError, match="outside the 63 vertices"):
            mesh.mesh_adjacency(torch.from_numpy(bad).cuda(), len(v))
    for bad in (float("nan"), float("inf"), -float("inf")):
        vb = m["vertices"].clone()
        vb[17, 1] = bad
        with pytest.raises(ValueError, match="vertices must be finite"):
            mesh.smooth_mesh(dict(m, vertices=vb), 2)
    for kw in (dict(iterations=0), dict(iterations=1001), dict(iterations=2, lam=0.0), dict(iterations=2, mu=0.5),
               dict(iterations=2, max_move=-1.0)):
        with pytest.raises(ValueError, match="must be"):
            mesh.smooth_mesh(m, **kw)


def _raw_adjacency(lib, faces, nv):
    """The adjacency through the entry points alone (no segment of these meshes is longer than CDS_MESH_ADJ_SMALL)."""
    tf, nf = torch.from_numpy(np.ascontiguousarray(faces)).cuda(), len(faces)
    count = torch.zeros(nv, dtype=torch.int32, device="cuda")
    assert lib.cds_mesh_adj_count(tf.data_ptr(), nf, nv, count.data_ptr(), None) == 0
    assert int(count.max()) <= lib.cds_mesh_adj_small() == mesh.ADJ_SMALL
    start = torch.zeros(nv + 1, dtype=torch.int32, device="cuda")
    start[1:] = torch.cumsum(count, 0)
    ne = int(start[-1])
    nbr = torch.full((ne,), -7, dtype=torch.int32, device="cuda")
    cursor = torch.zeros(nv, dtype=torch.int32, device="cuda")
    assert lib.cds_mesh_adj_fill(tf.data_ptr(), nf, nv, start.data_ptr(), cursor.data_ptr(), nbr.data_ptr(), ne, None) == 0
    deg = torch.full((nv,), -7, dtype=torch.int32, device="cuda")
    flags = torch.full((nv,), 77, dtype=torch.uint8, device="cuda")
    assert lib.cds_mesh_adj_finish(nv, start.data_ptr(), nbr.data_ptr(), ne, deg.data_ptr(), flags.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return {"start": start, "degree": deg, "neighbors": nbr, "boundary": (flags & 1) != 0, "isolated": (flags & 2) != 0}, cursor, count


def test_entry_points_skip_what_the_wrapper_never_sends():
    """A face with an index outside the vertices adds nothing: the adjacency is that of the mesh without it.  A step through the
    entry point equals the restatement's.  in == out, null pointers and sizes out of range are CDS_EINVAL before any launch; empty
    inputs return 0."""
    lib = _lib.load()
    v, c, good = S.sphere()
    nv = len(v)
    bad = np.insert(good, [0, 700, 700, 4568], np.array([[0, 1, nv], [-1, 0, 4], [3, 2 ** 31 - 1, 5], [nv + 7, 2, 3]], np.int32), axis=0)
    want = _adj("sphere")
    for faces in (good, bad):
        adj, cursor, count = _raw_adjacency(lib, faces, nv)
        _check_adjacency(adj, want, "through the entry points")
        assert torch.equal(cursor, count)
    tv = torch.from_numpy(v).cuda()
    out = torch.zeros_like(tv)
    step = lib.cds_mesh_smooth_step_f32
    a = (adj["start"].data_ptr(), adj["degree"].data_ptr(), adj["neighbors"].data_ptr())
    assert step(tv.data_ptr(), out.data_ptr(), nv, *a, 0.5, None) == 0
    _same(out.cpu().numpy(), S.step(v, want, 0.5), "one step through the entry point")
    move2 = torch.zeros(nv, dtype=torch.float64, device="cuda")
    flag = torch.full((nv,), 9, dtype=torch.uint8, device="cuda")
    lim = lib.cds_mesh_smooth_limit_f32
    assert lim(tv.data_ptr(), out.data_ptr(), nv, 0.0, move2.data_ptr(), flag.data_ptr(), None) == 0
    wpos, wn2, wcl = S.limit(v, S.step(v, want, 0.5), 0.0)
    _same(out.cpu().numpy(), wpos, "no limit: the positions stay")
    _same(move2.cpu().numpy(), wn2, "squared moves")
    assert not flag.any()
    p = torch.zeros(64, dtype=torch.int64, device="cuda").data_ptr()
    E = _lib.EINVAL
    assert step(p, p, 2, p, p, p, 0.5, None) == E                                                   # in == out
    assert step(None, p + 64, 2, p, p, p, 0.5, None) == E and step(p, None, 2, p, p, p, 0.5, None) == E
    assert step(p, p + 64, 2, None, p, p, 0.5, None) == E and step(p, p + 64, 2, p, None, p, 0.5, None) == E
    assert step(p, p + 64, 2, p, p, None, 0.5, None) == E and step(p, p + 64, -1, p, p, p, 0.5, None) == E
    assert step(p, p + 64, 2 ** 31, p, p, p, 0.5, None) == E and step(p, p + 64, 2, p, p, p, float("nan"), None) == E
    assert step(p, p + 64, 2, p, p, p, float("inf"), None) == E and step(None, None, 0, None, None, None, 0.5, None) == 0
    assert lim(p, p, 2, 1.0, p, p, None) == E and lim(None, p + 64, 2, 1.0, p, p, None) == E and lim(p, None, 2, 1.0, p, p, None) == E
    assert lim(p, p + 64, 2, 1.0, None, p, None) == E and lim(p, p + 64, 2, 1.0, p, None, None) == E
    assert lim(p, p + 64, 2, -1.0, p, p, None) == E and lim(p, p + 64, 2, float("nan"), p, p, None) == E
    assert lim(p, p + 64, 2, float("inf"), p, p, None) == E and lim(p, p + 64, -1, 1.0, p, p, None) == E
    assert lim(p, p + 64, 2 ** 31, 1.0, p, p, None) == E and lim(None, None, 0, 1.0, None, None, None) == 0
    cnt, fill, fin = lib.cds_mesh_adj_count, lib.cds_mesh_adj_fill, lib.cds_mesh_adj_finish
    assert cnt(None, 1, 8, p, None) == E and cnt(p, 1, 8, None, None) == E and cnt(p, -1, 8, p, None) == E
    assert cnt(p, 1, 2 ** 31, p, None) == E and cnt(p, 2 ** 31 // 6 + 1, 8, p, None) == E and cnt(p, 1, -1, p, None) == E
    assert cnt(None, 0, 8, None, None) == 0 and cnt(None, 1, 0, None, None) == 0
    assert fill(None, 1, 8, p, p, p, 6, None) == E and fill(p, 1, 8, None, p, p, 6, None) == E and fill(p, 1, 8, p, None, p, 6, None) == E
    assert fill(p, 1, 8, p, p, None, 6, None) == E and fill(p, 1, 8, p, p, p, 7, None) == E and fill(p, 1, 8, p, p, p, -1, None) == E
    assert fill(p, 2 ** 31 // 6 + 1, 8, p, p, p, 6, None) == E and fill(p, -1, 8, p, p, p, 6, None) == E
    assert fill(None, 0, 8, None, None, None, 0, None) == 0 and fill(None, 1, 8, None, None, None, 0, None) == 0
    assert fin(8, None, p, 6, p, p, None) == E and fin(8, p, None, 6, p, p, None) == E and fin(8, p, p, 6, None, p, None) == E
    assert fin(8, p, p, 6, p, None, None) == E and fin(-1, p, p, 6, p, p, None) == E and fin(8, p, p, 2 ** 31, p, p, None) == E
    assert fin(2 ** 31, p, p, 6, p, p, None) == E and fin(0, None, None, 0, None, None, None) == 0
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------------- end to end
def _no_smooth(*a, **k):
    raise AssertionError("smooth_mesh ran without --mesh_smooth")


def test_mesh_scan_and_command_line(tmp_path, capsys, monkeypatch):
    """The synthetic scan of test_mesh_gpu (3 views of 24 x 40): mesh_scan(smooth=5) writes smooth_mesh of the mesh it writes
    without; clean, smooth, simplify through mesh_scan are the three library calls in that order; mesh.main with --mesh_voxel and
    with --from_mesh write the same file for the same mesh; without the option nothing of this runs and no byte changes."""
    scan, pairs = _write_outputs(tmp_path)
    out = tmp_path / "out"
    kw = dict(thres_view=1)
    cli = ["--testpath", str(tmp_path / "in"), "--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--thres_view", "1",
           "--mesh_voxel", str(VOXEL)]
    # the parts this step does not touch: the fusion pass, mesh_views, the writer; clean_mesh for a saved file
    views: list = []
    fusion.filter_depth(str(pairs), str(scan), None, collect=views, **kw)
    raw = mesh.mesh_views(views, VOXEL)[0]
    untouched = str(tmp_path / "untouched_mesh.ply")
    mesh.write_mesh_ply(untouched, *(raw[k].cpu().numpy() for k in ("vertices", "colors", "faces")))
    plain = str(tmp_path / "plain_mesh.ply")
    with monkeypatch.context() as mp:
        mp.setattr(mesh, "smooth_mesh", _no_smooth)
        info0 = mesh.mesh_scan(str(pairs), str(scan), plain, VOXEL, **kw)
        zero = mesh.mesh_scan(str(pairs), str(scan), str(tmp_path / "zero_mesh.ply"), VOXEL, smooth=0, **kw)
        mesh.main(cli)
        assert filecmp.cmp(str(out / "scan1_mesh.ply"), untouched, shallow=False)
        saved = str(tmp_path / "saved_mesh.ply")
        os.replace(out / "scan1_mesh.ply", saved)
        mesh.main(["--from_mesh", saved, "--outdir", str(out), "--testlist", str(tmp_path / "list.txt")])
        cleaned = mesh.clean_mesh(_upload(*mesh.read_mesh_ply(saved)))[0]
        mesh.write_mesh_ply(str(tmp_path / "cleaned_mesh.ply"), *(cleaned[k].cpu().numpy() for k in ("vertices", "colors", "faces")))
        assert filecmp.cmp(str(out / "scan1_mesh.ply"), str(tmp_path / "cleaned_mesh.ply"), shallow=False)
    assert filecmp.cmp(plain, untouched, shallow=False) and filecmp.cmp(str(tmp_path / "zero_mesh.ply"), untouched, shallow=False)
    assert sorted(info0) == sorted(zero) == ["blocks", "cloud", "faces", "mesh", "vertices"]
    arrays = mesh.read_mesh_ply(plain)
    assert len(arrays[2]) > 0
    # mesh_scan(smooth=5) against smooth_mesh of the mesh that mesh_scan hands back, and against the restatement
    smoothed, sinfo = mesh.smooth_mesh(info0["mesh"], 5)
    lib_ply = str(tmp_path / "lib_mesh.ply")
    mesh.write_mesh_ply(lib_ply, *(smoothed[k].cpu().numpy() for k in ("vertices", "colors", "faces")))
    direct = str(tmp_path / "direct_mesh.ply")
    info = mesh.mesh_scan(str(pairs), str(scan), direct, VOXEL, smooth=5, **kw)
    assert filecmp.cmp(direct, lib_ply, shallow=False) and not filecmp.cmp(direct, plain, shallow=False)
    assert info["smooth"] == dict(sinfo, limit=0.0) and info["blocks"] == info0["blocks"] and "clean" not in info
    wout, winfo = S.smooth(*arrays, 5)
    v, c, f = _check_file(direct)
    _same(v, wout["vertices"], "mesh_scan: vertices")
    _same(c, arrays[1], "mesh_scan: colors")
    _same(f, arrays[2], "mesh_scan: faces")
    assert sinfo == winfo and winfo["boundary"] > 0
    assert np.array_equal(info["mesh"]["vertices"].cpu().numpy().view(np.uint32), v.view(np.uint32))      # what render_scan gets
    # clean -> smooth -> simplify
    cell = 2.0 * VOXEL
    a, ia = mesh.clean_mesh(info0["mesh"], 5, 0)
    b, ib = mesh.smooth_mesh(a, 3, 0.6, -0.5, 0.02 * VOXEL)
    d, id_ = mesh.simplify_mesh(b, cell, "quadric")
    chain = str(tmp_path / "chain_mesh.ply")
    mesh.write_mesh_ply(chain, *(d[k].cpu().numpy() for k in ("vertices", "colors", "faces")))
    three = str(tmp_path / "three_mesh.ply")
    info = mesh.mesh_scan(str(pairs), str(scan), three, VOXEL, min_component=5, simplify=cell, smooth=3, smooth_lambda=0.6,
                          smooth_mu=-0.5, smooth_max_move=0.02 * VOXEL, **kw)
    assert filecmp.cmp(three, chain, shallow=False)
    rounds = {"rounds": 0}                                               # the hook passes of the labelling vary from run to run
    assert dict(info["clean"], **rounds) == dict(ia, **rounds) and ia["faces"][1] > 0
    assert info["smooth"] == dict(ib, limit=0.02 * VOXEL) and info["simplify"] == id_ and ib["clamped"] > 0
    # the command line: --mesh_voxel, in this process and in a child, and --from_mesh on the saved mesh
    capsys.readouterr()
    res = mesh.main(cli + ["--mesh_smooth", "5"])
    line = capsys.readouterr().out
    assert res["scan1"]["smooth"] == dict(winfo, limit=0.0) and filecmp.cmp(str(out / "scan1_mesh.ply"), direct, shallow=False)
    assert (f"smoothed 5 iterations (lambda 0.5, mu -0.53): {winfo['boundary']} boundary, {winfo['isolated']} isolated vertices, "
            f"largest move {winfo['max_move']:.6g}") in line and "clamped" not in line
    os.remove(out / "scan1_mesh.ply")
    stdout = _child("cds_mvsnet_amd.mesh", cli + ["--mesh_smooth", "5"])
    assert filecmp.cmp(str(out / "scan1_mesh.ply"), direct, shallow=False) and "smoothed 5 iterations" in stdout
    os.remove(out / "scan1_mesh.ply")
    res = mesh.main(["--from_mesh", saved, "--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--mesh_smooth", "5"])
    assert filecmp.cmp(str(out / "scan1_mesh.ply"), direct, shallow=False)
    assert res["scan1"]["smooth"] == dict(winfo, limit=0.0) and "clean" not in res["scan1"]
    res = mesh.main(["--from_mesh", saved, "--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--mesh_smooth", "3",
                     "--mesh_smooth_lambda", "0.6", "--mesh_smooth_mu", "-0.5", "--mesh_smooth_max_move", str(0.02 * VOXEL),
                     "--mesh_min_component", "5", "--mesh_simplify", str(cell)])
    assert filecmp.cmp(str(out / "scan1_mesh.ply"), chain, shallow=False)
    assert f"{ib['clamped']} clamped to {0.02 * VOXEL:g}" in capsys.readouterr().out
    assert filecmp.cmp(saved, untouched, shallow=False)                                             # the source is not touched


def test_infer_smooth_and_render(tmp_path, capsys):
    """infer --fuse --mesh_voxel --mesh_smooth 5 --render_mesh on a scene of test_mvs_io._write_scene (3 views of 128 x 160, an
    untrained network, the loose settings of test_mesh_gpu.test_infer_fuse_mesh): the mesh file is smooth_mesh of the file of the
    run without the option (in which smooth_mesh is not called, and which equals the mesh of the parts this step does not touch),
    every other file is that run's, and depth_mesh is render_scan of the smoothed file."""
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanA", 3, 128, 160, seed=3)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("scanA\n")
    base = ["--testpath", root, "--testlist", lst, "--num_view", "3", "--max_h", "128", "--max_w", "160", "--interval_scale", "1.0",
            "--fuse", "--mesh_voxel", "10"] + FUSE
    plain = str(tmp_path / "plain")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(mesh, "smooth_mesh", _no_smooth)
        infer.main(base + ["--outdir", plain])
    views: list = []
    fusion.filter_depth(os.path.join(root, "scanA"), os.path.join(plain, "scanA"), None, collect=views, method="dynamic",
                        conf=(0.0, 0.0, 0.0), dist_base=2.0, rel_base=0.02, n_views=(1, 10))
    raw = mesh.mesh_views(views, 10.0)[0]
    untouched = str(tmp_path / "untouched_mesh.ply")
    mesh.write_mesh_ply(untouched, *(raw[k].cpu().numpy() for k in ("vertices", "colors", "faces")))
    assert filecmp.cmp(os.path.join(plain, "scanA_mesh.ply"), untouched, shallow=False)
    arrays = mesh.read_mesh_ply(untouched)
    wout, winfo = S.smooth(*arrays, 5)
    out = str(tmp_path / "smooth")
    capsys.readouterr()
    infer.main(base + ["--outdir", out, "--mesh_smooth", "5", "--render_mesh"])
    lines = capsys.readouterr().out.splitlines()
    v, c, f = _check_file(os.path.join(out, "scanA_mesh.ply"))
    _same(v, wout["vertices"], "infer: vertices")
    _same(c, arrays[1], "infer: colors")
    _same(f, arrays[2], "infer: faces")
    line = [ln for ln in lines if "scanA_mesh.ply" in ln]
    assert line and f"smoothed 5 iterations (lambda 0.5, mu -0.53): {winfo['boundary']} boundary" in line[0]
    for name in _tree(plain):
        if name != "scanA_mesh.ply":
            assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    scan = os.path.join(out, "scanA")
    render.render_scan(scan, os.path.join(out, "scanA_mesh.ply"), os.path.join(root, "scanA"), subdir="again")
    render.render_scan(scan, untouched, os.path.join(root, "scanA"), subdir="rough")
    differ = 0
    for i in range(3):
        a = mvs_io.read_pfm(os.path.join(scan, "depth_mesh", f"{i:08d}.pfm"))[0]
        b = mvs_io.read_pfm(os.path.join(scan, "again", f"{i:08d}.pfm"))[0]
        d = mvs_io.read_pfm(os.path.join(scan, "rough", f"{i:08d}.pfm"))[0]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (a > 0).any()
        differ += int((a.view(np.uint32) != d.view(np.uint32)).sum())
    assert differ > 0                                                    # the maps are those of the smoothed mesh
    print(f"{winfo['vertices']} vertices, largest move {winfo['max_move']:.3f}; {differ} pixels of depth_mesh change")


def test_sphere_from_26_cameras_gets_closer_to_the_sphere():
    """The 26-camera sphere of test_mesh_weighted_gpu through mesh_views at its unweighted defaults: 10 iterations on the device
    equal the restatement on the same extracted mesh, and the rms distance of the vertices to the sphere falls."""
    sc, views = _sphere_records()
    s = sc["voxel"]
    m, vol = mesh.mesh_views(views, s, 2.5 * s, 2)
    v, c, f = (m[k].cpu().numpy() for k in ("vertices", "colors", "faces"))
    wout, winfo = S.smooth(v, c, f, 10)
    got, info = mesh.smooth_mesh(m, 10)
    _same(got["vertices"].cpu().numpy(), wout["vertices"], "sphere scene: vertices")
    assert info == winfo and torch.equal(got["faces"], m["faces"]) and torch.equal(got["colors"], m["colors"])
    before, after = W.radial_error(v, sc), W.radial_error(wout["vertices"], sc)
    print(f"sphere scene, {len(v)} vertices: rms {before[0]:.4f} -> {after[0]:.4f} voxels, max {before[1]:.4f} -> {after[1]:.4f}; "
          f"largest move {info['max_move'] / s:.3f} voxels")
    assert after[0] < before[0]
    tp = M.topology(f, len(v))
    assert tp["euler"] == 2 and (tp["edge_uses"] == 2).all() and info["boundary"] == 0 and info["isolated"] == 0
