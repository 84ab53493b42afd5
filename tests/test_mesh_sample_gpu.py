"""The kernels of csrc/mesh_sample.hip against the numpy restatement of their rule (mesh_sample_ref.py): positions
bit for bit, colours, face ids and the info exactly.  Then the errors, determinism, and the ways to a sampled surface:
dtu_eval --sample_faces and tt_eval --sample_faces against their oracles, and python -m cds_mvsnet_amd.mesh --mesh_sample."""
import argparse
import filecmp
import functools
import json
import os

import numpy as np
import pytest
import torch

import dtu_eval_ref as D
import mesh_clean_ref as C
import mesh_ref as M
import mesh_sample_ref as R
import tt_eval_ref as T
from cds_mvsnet_amd import _lib, dtu_eval, fusion, mesh, pointcloud, synth, tt_eval
from test_dtu_eval_cpu import _dtu_layout
from test_dtu_eval_gpu import _assert_stats
from test_mesh_gpu import VOXEL, _child, _write_outputs
from test_tt_eval_cpu import _tt_layout

pytestmark = pytest.mark.gpu

TRI345 = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], np.float32)
F1 = np.array([[0, 1, 2]], np.int32)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}, expected {want.dtype} {want.shape}"
    if not np.array_equal(_bits(got), _bits(want)):
        bad = np.nonzero((_bits(got) != _bits(want)).reshape(len(got), -1).any(1))[0]
        raise AssertionError(f"{what} differs in {len(bad)} of {len(got)} rows, first at {bad[:5].tolist()}: {got[bad[:3]].tolist()} "
                             f"expected {want[bad[:3]].tolist()}")


def _upload(v, c, f):
    return {"vertices": torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(),
            "colors": torch.from_numpy(np.ascontiguousarray(c, np.uint8)).cuda(),
            "faces": torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()}


def _sphere():
    m = M.analytic_case("sphere")[1]
    return m["vertices"], m["colors"], m["faces"]


def _random():
    rng = np.random.default_rng(4)
    return rng.uniform(0, 6, (500, 3)).astype(np.float32), rng.integers(0, 256, (500, 3)).astype(np.uint8), C.random_faces(500, 2000, seed=2)


def _with_nan_faces(where):
    """The small faces around a large one, with faces that hold a NaN corner (n = 0: equal neighbouring offsets)."""
    v, c, f = R.small_faces_around_a_large_one()
    v = np.concatenate([v, np.array([[np.nan, 0, 0]], np.float32)])
    c = np.concatenate([c, c[:1]])
    bad = np.array([[0, 1, len(v) - 1]], np.int32)
    f = {"first": lambda: np.concatenate([bad, f]), "last": lambda: np.concatenate([f, bad]),
         "middle": lambda: np.concatenate([f[:400], np.repeat(bad, 300, 0), f[400:]]),
         "all": lambda: np.concatenate([bad, f[:400], np.repeat(bad, 300, 0), f[400:], bad])}[where]()
    return v, c, np.ascontiguousarray(f, np.int32)


def _one_large_face():
    return TRI345, np.array([[0, 0, 255], [0, 255, 255], [255, 0, 9]], np.uint8), F1


MESHES = {"cube": (R.cube, 0.5), "cube_fine": (R.cube, 0.2), "sphere": (_sphere, 0.4), "random": (_random, 0.25),
          "large_among_small": (R.small_faces_around_a_large_one, 1.0),
          "nan_first": (lambda: _with_nan_faces("first"), 1.0), "nan_last": (lambda: _with_nan_faces("last"), 1.0),
          "nan_middle": (lambda: _with_nan_faces("middle"), 1.0), "nan_all": (lambda: _with_nan_faces("all"), 1.0),
          "one_face": (lambda: tuple(a if i < 2 else a[:1] for i, a in enumerate(R.cube())), 0.5),
          "sparse": (lambda: C.isolated_triangles(70, n_vertices=100003, seed=7), 0.3),
          "n2048": (_one_large_face, 5.0 / 2048)}


@functools.lru_cache(maxsize=None)
def _want(name):
    """The restatement's result for a named mesh; computed once, not to be modified."""
    make, spacing = MESHES[name]
    return R.sample(*make(), spacing)


def _check(v, c, f, spacing, want, what):
    wout, winfo, wn = want
    got, info = mesh.sample_mesh(_upload(v, c, f), spacing)
    out = {}
    for k in ("points", "colors", "face"):
        assert got[k].is_cuda and got[k].is_contiguous()
        out[k] = got[k].cpu().numpy()
    assert info == winfo, f"{what}: {info}, expected {winfo}"
    _same(out["face"], wout["face"], f"{what}: face ids")
    _same(out["colors"], wout["colors"], f"{what}: colours")
    _same(out["points"], wout["points"], f"{what}: points")
    return out, info, wn


def _named(name):
    make, spacing = MESHES[name]
    return _check(*make(), spacing, _want(name), name)


# ---------------------------------------------------------------------------------------------------------------- the cases
def test_cube():
    out, info, n = _named("cube")
    assert info == {"faces": 12, "points": 1728, "max_n": 12, "skipped": 0}
    out, info, n = _named("cube_fine")
    assert info["points"] == 10092


def test_sphere_and_random_faces():
    out, info, n = _named("sphere")
    assert set(range(1, 5)) <= set(n.tolist()) and info["faces"] == 4568             # many faces, each of a few samples
    out, info, n = _named("random")
    assert info["max_n"] > 20 and n.min() >= 1


def test_one_large_face_among_small_ones():
    out, info, n = _named("large_among_small")
    assert sorted(n.tolist())[-2:] == [1, 300] and n[500] == 300 and info["points"] == 1000 + 90000


@pytest.mark.parametrize("where", ["first", "last", "middle", "all"])
def test_faces_without_samples(where):
    out, info, n = _named(f"nan_{where}")
    assert info["skipped"] == {"first": 1, "last": 1, "middle": 300, "all": 302}[where] and info["points"] == 91000
    assert np.isfinite(out["points"]).all()


def test_a_face_of_four_million_samples():
    """n = 2048: the integer square root at every row boundary k = r^2 - 1, r^2."""
    out, info, n = _named("n2048")
    assert info == {"faces": 1, "points": 4194304, "max_n": 2048, "skipped": 0}


def test_one_face_no_face_and_many_unreferenced_vertices(monkeypatch):
    _named("one_face")
    out, info, n = _named("sparse")
    assert info["faces"] == 70
    with monkeypatch.context() as mp:
        def no_launch():
            raise AssertionError("the library was loaded: a launch was about to happen")
        mp.setattr(mesh._lib, "load", no_launch)
        for nv in (0, 5):
            v, c, f = np.zeros((nv, 3), np.float32), np.zeros((nv, 3), np.uint8), np.zeros((0, 3), np.int32)
            out, info, n = _check(v, c, f, 1.0, R.sample(v, c, f, 1.0), f"F = 0, V = {nv}")
            assert out["points"].shape == (0, 3) and info == {"faces": 0, "points": 0, "max_n": 0, "skipped": 0}
    # every face skipped: counted, nothing emitted
    v = np.array([[np.inf, 0, 0], [0, 0, 0], [1, 0, 0]], np.float32)
    out, info, n = _check(v, np.zeros((3, 3), np.uint8), F1, 1.0, R.sample(v, np.zeros((3, 3), np.uint8), F1, 1.0), "all skipped")
    assert info == {"faces": 1, "points": 0, "max_n": 0, "skipped": 1}


def test_exact_boundaries_on_the_device():
    """Rule 1 where the guess and the test can disagree: the 3-4-5 triangle at spacings around 1."""
    col = np.zeros((3, 3), np.uint8)
    for spacing, n in ((1.0, 5), (0.5, 10), (float(np.nextafter(1.0, 0)), 6), (float(np.nextafter(1.0, 2)), 5), (5.0 / 32768, 32768)):
        if n > 2048:                                                     # the count alone: 2^30 samples are not made here
            lib, m = _lib.load(), _upload(TRI345, col, F1)
            cnt, cnt2 = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
            assert lib.cds_mesh_sample_count(m["vertices"].data_ptr(), 3, m["faces"].data_ptr(), 1, spacing, cnt.data_ptr(),
                                             cnt2.data_ptr(), None) == 0
            assert int(cnt) == n == int(R.counts(TRI345, F1, spacing)[0]) and int(cnt2) == n * n
            continue
        got, info = mesh.sample_mesh(_upload(TRI345, col, F1), spacing)
        assert info["max_n"] == n == int(R.counts(TRI345, F1, spacing)[0]) and info["points"] == n * n


# ------------------------------------------------------------------------------------------------------------------- errors
def test_errors():
    m = _upload(*R.cube())
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="spacing must be positive"):
            mesh.sample_mesh(m, bad)
    big = np.array([[0, 0, 0], [1e6, 0, 0], [0, 1e6, 0]], np.float32)
    with pytest.raises(ValueError, match="more than 32768 subdivisions"):
        mesh.sample_mesh(_upload(big, np.zeros((3, 3), np.uint8), F1), 1.0)
    with pytest.raises(ValueError, match="1728 points.*raise the spacing or simplify"):
        mesh.sample_mesh(m, 0.5, max_points=100)
    assert mesh.sample_mesh(m, 0.5, max_points=1728)[1]["points"] == 1728
    for k in ("vertices", "colors", "faces"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mesh.sample_mesh(dict(m, **{k: m[k].cpu()}), 0.5)
    with pytest.raises(ValueError, match="outside the 8 vertices"):
        mesh.sample_mesh(dict(m, faces=torch.tensor([[0, 1, 8]], dtype=torch.int32, device="cuda")), 0.5)
    with pytest.raises(ValueError, match="faces must be an int32"):
        mesh.sample_mesh(dict(m, faces=m["faces"].long()), 0.5)


def test_entry_points_refuse_bad_arguments_and_skip_faces_outside_the_vertices():
    lib, E = _lib.load(), _lib.EINVAL
    assert lib.cds_mesh_sample_max_n() == R.MAX_N == mesh.MAX_SAMPLE_N
    p = torch.zeros(64, dtype=torch.int64, device="cuda").data_ptr()
    cnt = lib.cds_mesh_sample_count
    assert cnt(p, 8, p, -1, 1.0, p, p, None) == E and cnt(p, 8, p, 2 ** 31, 1.0, p, p, None) == E
    assert cnt(p, 2 ** 31, p, 1, 1.0, p, p, None) == E and cnt(p, -1, p, 1, 1.0, p, p, None) == E
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert cnt(p, 8, p, 1, bad, p, p, None) == E
    assert cnt(None, 8, p, 1, 1.0, p, p, None) == E and cnt(p, 8, None, 1, 1.0, p, p, None) == E
    assert cnt(p, 8, p, 1, 1.0, None, p, None) == E and cnt(p, 8, p, 1, 1.0, p, None, None) == E
    assert cnt(None, 8, None, 0, 1.0, None, None, None) == 0
    emit = lib.cds_mesh_sample_emit
    assert emit(p, p, 8, p, 1, p, p, -1, p, p, p, None) == E and emit(p, p, 8, p, 1, p, p, 2 ** 31, p, p, p, None) == E
    assert emit(p, p, 8, p, 2 ** 31, p, p, 1, p, p, p, None) == E and emit(p, p, -1, p, 1, p, p, 1, p, p, p, None) == E
    for i in (0, 1, 3, 5, 6, 8, 9, 10):
        args = [p, p, 8, p, 1, p, p, 1, p, p, p, None]
        args[i] = None
        assert emit(*args) == E, i
    assert emit(p, p, 8, p, 1, p, p, 1, p + 4, p, p, None) == E                         # a misaligned output
    assert emit(None, None, 8, None, 0, None, None, 0, None, None, None, None) == 0
    assert emit(None, None, 8, None, 1, None, None, 0, None, None, None, None) == 0
    # faces with an index outside the vertices: the count is 0; an emit that is handed counts for them writes nothing there
    v, c, good = _random()
    nv = len(v)
    bad = np.insert(good, [0, 700, 2000], np.array([[0, 1, nv], [-1, 0, 4], [3, 2 ** 31 - 1, 5]], np.int32), axis=0)
    valid = np.ones(len(bad), bool)
    valid[[0, 701, 2002]] = False
    assert np.array_equal(bad[valid], good)
    m, nf = _upload(v, c, bad), len(bad)
    n = torch.full((nf,), 7, dtype=torch.int32, device="cuda")
    n2 = torch.full((nf,), 7, dtype=torch.int64, device="cuda")
    assert cnt(m["vertices"].data_ptr(), nv, m["faces"].data_ptr(), nf, 0.25, n.data_ptr(), n2.data_ptr(), None) == 0
    want_n = R.counts(v, good, 0.25)
    assert np.array_equal(n.cpu().numpy()[valid], want_n) and (n.cpu().numpy()[~valid] == 0).all()
    assert np.array_equal(n2.cpu().numpy(), n.cpu().numpy().astype(np.int64) ** 2)
    n[~torch.from_numpy(valid).cuda()] = 2                                             # as if they had four samples each
    n2 = n.long() * n.long()
    ends = torch.cumsum(n2, 0)
    total = int(ends[-1])
    pts = torch.full((total, 3), -7.0, dtype=torch.float32, device="cuda")
    col = torch.full((total, 3), 9, dtype=torch.uint8, device="cuda")
    fid = torch.full((total,), -5, dtype=torch.int32, device="cuda")
    assert emit(m["vertices"].data_ptr(), m["colors"].data_ptr(), nv, m["faces"].data_ptr(), nf, n.data_ptr(), (ends - n2).data_ptr(),
                total, pts.data_ptr(), col.data_ptr(), fid.data_ptr(), None) == 0
    torch.cuda.synchronize()
    fid, pts, col = fid.cpu().numpy(), pts.cpu().numpy(), col.cpu().numpy()
    owner = np.repeat(np.arange(nf), n2.cpu().numpy())
    skipped = ~valid[owner]
    assert skipped.sum() == 12 and (fid[skipped] == -5).all() and (pts[skipped] == -7.0).all() and (col[skipped] == 9).all()
    wout = R.sample(v, c, good, 0.25)[0]
    _same(pts[~skipped], wout["points"], "points next to skipped faces")
    _same(col[~skipped], wout["colors"], "colours next to skipped faces")
    assert np.array_equal(np.nonzero(valid)[0][wout["face"]], fid[~skipped])


def test_two_runs_are_equal_on_a_side_stream_too():
    make, spacing = MESHES["large_among_small"]
    m = _upload(*make())
    (a, ia), (b, ib) = mesh.sample_mesh(m, spacing), mesh.sample_mesh(m, spacing)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c, ic = mesh.sample_mesh(m, spacing)
    torch.cuda.current_stream().wait_stream(s)
    assert ia == ib == ic
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) and torch.equal(a[k].view(torch.uint8), c[k].view(torch.uint8))


# -------------------------------------------------------------------------------------------------------------- the scorers
def test_dtu_eval_scores_the_surface_of_a_mesh(tmp_path, capsys):
    """The height field of the synthetic DTU scene as a mesh of 9 x 7 vertices.  --dst 0.5 (so the default spacing is 0.5) and
    --max-dist 0.5 keep the oracle quick and make completeness tell samples from vertices: a vertex covers a disc of radius 0.5
    of a surface whose vertices are 5 apart.  The oracle runs with MaxDistCP's block at the protocol's 60 and not at 3 max_dist:
    every point lies inside BB, so the blocks tile all of them whatever their side, and a distance below max_dist is found
    exactly with any block >= max_dist; the statistics keep only those (measured: the same figures, 2 s against 60 s)."""
    gt = synth.make_dtu_scene(20, 15, 0.2, 0.5, 2.0, plane_z=655.0)
    v, f = R.height_field_mesh(np.linspace(-20, 20, 9), np.linspace(-15, 15, 7), synth.fusion_surface)
    assert v.shape == (63, 3) and f.shape == (96, 3)
    c = np.random.default_rng(1).integers(0, 256, v.shape).astype(np.uint8)
    data, plydir = tmp_path / "MVS Data", tmp_path / "out"
    _dtu_layout(data, 9, gt)
    plydir.mkdir()
    mesh.write_mesh_ply(str(plydir / "scan9_mesh.ply"), v, c, f)
    base = ["--datapath", str(data), "--plydir", str(plydir), "--scans", "9", "--ply", "{scan}_mesh.ply", "--dst", "0.5",
            "--max-dist", "0.5", "--seed", "3"]
    loaded = dtu_eval.load_dtu_scan(str(data), 9)

    res = dtu_eval.main(base + ["--sample_faces", "--json", str(tmp_path / "s.json")])
    printed = capsys.readouterr().out
    got = json.load(open(tmp_path / "s.json"))
    wout, winfo, _ = R.sample(v, c, f, 0.5)
    want = D.point_compare(wout["points"], loaded, 0.5, pointcloud.thinning_order(winfo["points"], 3).numpy(), max_dist=0.5)
    g = got["scans"]["scan9"]
    assert g["n_sampled"] == winfo["points"] == g["n_points"] and g["n_faces"] == 96 and got["settings"]["sample_faces"] == 0.5
    assert f"[{winfo['points']} samples of 96 faces]" in printed
    assert g["n_thinned"] == int(want["keep"].sum()) and g["n_in_mask"] == int(want["data_in_mask"].sum())
    _assert_stats(g, want)
    assert res["scans"]["scan9"]["comp_n"] == g["comp_n"]

    plain = dtu_eval.main(base + ["--json", str(tmp_path / "v.json")])
    printed = capsys.readouterr().out
    vg = json.load(open(tmp_path / "v.json"))
    assert "samples of" not in printed and "sample_faces" not in vg["settings"] and "n_sampled" not in vg["scans"]["scan9"]
    vwant = D.point_compare(v, loaded, 0.5, pointcloud.thinning_order(len(v), 3).numpy(), max_dist=0.5)
    assert vg["scans"]["scan9"]["n_points"] == 63
    _assert_stats(vg["scans"]["scan9"], vwant)
    print(f"comp_n: {g['comp_n']} of {g['n_above_plane']} STL points above the plane with --sample_faces, "
          f"{vg['scans']['scan9']['comp_n']} from the vertices alone; comp {g['comp']:.4f} against {vg['scans']['scan9']['comp']:.4f}")
    assert g["comp_n"] >= 10 * vg["scans"]["scan9"]["comp_n"] > 0
    # an explicit spacing
    res = dtu_eval.main(base + ["--sample_faces", "1.0"])
    assert res["scans"]["scan9"]["n_sampled"] == R.sample(v, c, f, 1.0)[1]["points"] and res["settings"]["sample_faces"] == 1.0
    # a cloud under the flag: an error that names the file
    fusion.write_ply(str(plydir / "scan9.ply"), v, c)
    with pytest.raises(SystemExit, match="scan9.ply"):
        dtu_eval.main(base[:6] + ["--sample_faces"])
    with pytest.raises(SystemExit):
        dtu_eval.main(base + ["--sample_faces", "-1"])


def test_tt_eval_scores_the_surface_of_a_mesh(tmp_path, capsys):
    """A coarse triangulation (9 x 9 vertices) of the synthetic T&T surface, placed by the scene's own alignment."""
    sc = synth.make_tt_scene(n_gt=6000, n_pred=10, tau=0.02, hole_radius=4.0, seed=4)
    tau, centre = sc["tau"], np.array([1.5, -0.8, 0.6])
    half = 0.5 * (round(np.sqrt(6000)) - 1) * tau / 2.0
    g = np.linspace(-half, half, 9)
    v, f = R.height_field_mesh(centre[0] + g, centre[1] + g, lambda x, y: synth.tt_surface(x, y, half, centre))
    inv = np.linalg.inv(sc["trans"])
    v = (v.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)                  # into the prediction's frame
    c = np.zeros_like(v, dtype=np.uint8)
    data, out = tmp_path / "data", tmp_path / "out"
    _tt_layout(data, "MyGarden", sc)
    out.mkdir()
    mesh.write_mesh_ply(str(out / "MyGarden.ply"), v, c, f)
    base = ["--datapath", str(data), "--plydir", str(out), "--scenes", "MyGarden", "--tau", str(tau), "--no-register"]
    plain = tt_eval.main(base + ["--json", str(tmp_path / "v.json")])
    printed = capsys.readouterr().out
    vj = json.load(open(tmp_path / "v.json"))
    assert "samples of" not in printed and "sample_faces" not in vj["settings"] and "n_sampled" not in vj["scenes"]["MyGarden"]
    vwant = T.evaluate(v, sc["gt"], sc["crop"], sc["trans"], tau, do_register=False)
    pv = plain["scenes"]["MyGarden"]
    assert pv["n_pred"] == 81 and pv["n_pred_sampled"] == vwant["n_pred_sampled"] and abs(pv["recall"] - vwant["recall"]) <= 1e-3
    res = tt_eval.main(base + ["--sample_faces", "--json", str(tmp_path / "s.json")])
    printed = capsys.readouterr().out
    sj = json.load(open(tmp_path / "s.json"))
    ps = res["scenes"]["MyGarden"]
    wout, winfo, _ = R.sample(v, c, f, tau / 2.0)
    swant = T.evaluate(wout["points"], sc["gt"], sc["crop"], sc["trans"], tau, do_register=False)
    assert ps["n_sampled"] == winfo["points"] == ps["n_pred"] and ps["n_faces"] == 128 and ps["sample_spacing"] == tau / 2.0
    assert sj["settings"]["sample_faces"] == "tau / 2" and f"[{winfo['points']} samples of 128 faces]" in printed
    assert ps["n_pred_sampled"] == swant["n_pred_sampled"] and abs(ps["recall"] - swant["recall"]) <= 1e-3
    print(f"recall {ps['recall']:.4f} with --sample_faces ({ps['n_sampled']} samples), {pv['recall']:.4f} from the 81 vertices")
    assert ps["recall"] > pv["recall"] + 0.25
    res = tt_eval.main(base + ["--sample_faces", str(tau)])
    assert res["scenes"]["MyGarden"]["n_sampled"] == R.sample(v, c, f, tau)[1]["points"] and res["settings"]["sample_faces"] == tau
    fusion.write_ply(str(out / "MyGarden.ply"), v, c)
    with pytest.raises(SystemExit, match="MyGarden.ply"):
        tt_eval.main(base + ["--sample_faces"])


# ----------------------------------------------------------------------------------------------------------- the mesh tool
def _surface_matches(surface_ply, mesh_ply, spacing):
    pts, col = fusion.read_ply(surface_ply)
    wout, winfo, _ = R.sample(*mesh.read_mesh_ply(mesh_ply), spacing)
    _same(np.ascontiguousarray(pts), wout["points"], "surface points")
    _same(np.ascontiguousarray(col), wout["colors"], "surface colours")
    return winfo


def test_mesh_command_line(tmp_path, capsys):
    v, c, f = R.cube()
    v2, c2, f2 = R.small_faces_around_a_large_one(50, 0.3, 20)
    saved = str(tmp_path / "saved_mesh.ply")
    mesh.write_mesh_ply(saved, np.concatenate([v, v2]), np.concatenate([c, c2]), np.concatenate([f, f2 + len(v)]).astype(np.int32))
    (tmp_path / "list.txt").write_text("scan1\n")
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    base = ["--from_mesh", saved, "--testlist", str(tmp_path / "list.txt")]
    def no_sampling(*args, **kw):
        raise AssertionError("sample_mesh ran without --mesh_sample")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(mesh, "sample_mesh", no_sampling)
        plain = mesh.main(base + ["--outdir", str(a)])
    assert "sample" not in plain["scan1"] and sorted(os.listdir(a)) == ["scan1_mesh.ply"]
    capsys.readouterr()
    res = mesh.main(base + ["--outdir", str(b), "--mesh_sample", "0.3"])
    line = capsys.readouterr().out
    assert sorted(os.listdir(b)) == ["scan1_mesh.ply", "scan1_surface.ply"]
    assert filecmp.cmp(a / "scan1_mesh.ply", b / "scan1_mesh.ply", shallow=False)
    winfo = _surface_matches(str(b / "scan1_surface.ply"), str(b / "scan1_mesh.ply"), 0.3)
    assert res["scan1"]["sample"] == dict(winfo, spacing=0.3) and f"surface sampled at 0.3: {winfo['points']} points" in line
    # after the simplification, as a child process
    stdout = _child("cds_mvsnet_amd.mesh", base + ["--outdir", str(b), "--mesh_sample", "0.25", "--mesh_simplify", "2.0"])
    winfo = _surface_matches(str(b / "scan1_surface.ply"), str(b / "scan1_mesh.ply"), 0.25)
    assert f"{winfo['points']} points" in stdout and "simplified" in stdout
    assert not filecmp.cmp(a / "scan1_mesh.ply", b / "scan1_mesh.ply", shallow=False)
    # argparse errors
    for bad in (["--outdir", str(b), "--testlist", str(tmp_path / "list.txt"), "--mesh_sample", "0.3"],
                base + ["--outdir", str(b), "--mesh_sample", "0"], base + ["--outdir", str(b), "--mesh_sample", "nan"]):
        with pytest.raises(SystemExit):
            mesh.main(bad)
    assert "--mesh_sample" in capsys.readouterr().err
    ap = argparse.ArgumentParser()
    mesh.add_mesh_args(ap)
    with pytest.raises(SystemExit):                                      # infer --mesh_sample without --mesh_voxel
        mesh.check_clean_args(ap, ap.parse_args(["--mesh_sample", "1.0"]), False)
    mesh.check_clean_args(ap, ap.parse_args(["--mesh_sample", "1.0", "--mesh_voxel", "2"]), True)
    assert ap.parse_args([]).mesh_sample is None


def test_mesh_scan_writes_the_surface(tmp_path, capsys):
    """--mesh_voxel --mesh_sample on the synthetic scan of test_mesh_gpu: the mesh file is the one of the run without the option,
    the surface file is the restatement's samples of it."""
    scan, pairs = _write_outputs(tmp_path)
    out = tmp_path / "out"
    cli = ["--testpath", str(tmp_path / "in"), "--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--thres_view", "1",
           "--mesh_voxel", str(VOXEL)]
    mesh.main(cli)
    plain = open(out / "scan1_mesh.ply", "rb").read()
    assert not os.path.exists(out / "scan1_surface.ply")
    res = mesh.main(cli + ["--mesh_sample", str(0.5 * VOXEL)])
    assert open(out / "scan1_mesh.ply", "rb").read() == plain
    winfo = _surface_matches(str(out / "scan1_surface.ply"), str(out / "scan1_mesh.ply"), 0.5 * VOXEL)
    assert res["scan1"]["sample"]["points"] == winfo["points"] > res["scan1"]["faces"] > 0
    assert f"{winfo['points']} points" in capsys.readouterr().out
