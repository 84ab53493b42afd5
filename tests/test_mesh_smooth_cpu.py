"""The numpy restatement of the smoothing rule (mesh_smooth_ref.py) against things known by construction: the noisy
analytic sphere gets smoother without shrinking, an open patch relaxes along its border and inside its plane, the limit holds; and
the parts of the public interface that need no GPU: argument checks, the header, the binding and the Makefile, the command-line
options, the printed line, and that nothing of it runs without the option."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_ref as M
import mesh_smooth_ref as S
from cds_mvsnet_amd import _lib, infer, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the sphere
def test_noisy_sphere_gets_smoother_and_keeps_its_volume():
    """Radial noise of 0.1 voxel on the analytic sphere (radius 6.37), 10 iterations at the defaults."""
    v, c, f = S.noisy_sphere()
    assert v.shape == (2286, 3) and f.shape == (4568, 3)
    rms0, ang0 = S.sphere_errors(v, f)
    vol0 = M.signed_volume(v, f)
    out, info = S.smooth(v, c, f, 10)
    flat, _ = S.smooth(v, c, f, 10, mu=0.0)
    rms1, ang1 = S.sphere_errors(out["vertices"], f)
    vol1, volf = M.signed_volume(out["vertices"], f), M.signed_volume(flat["vertices"], f)
    print(f"rms radial error {rms0:.4f} -> {rms1:.4f}, normals {ang0:.2f} -> {ang1:.2f} degrees off the radii, volume {vol0:.2f} -> "
          f"{vol1:.2f} (lambda|mu), {volf:.2f} (mu = 0); largest move {info['max_move']:.3f}")
    assert rms1 < 0.5 * rms0
    assert ang1 < ang0
    assert abs(vol1 - vol0) < 0.1 * abs(volf - vol0)
    before, after = M.topology(f, len(v)), M.topology(out["faces"], len(v))
    assert all(np.array_equal(before[k], after[k]) for k in before) and (before["edge_uses"] == 2).all()
    assert out["faces"] is not None and np.array_equal(out["faces"], f) and out["colors"] is c
    assert info == {"iterations": 10, "lam": 0.5, "mu": -0.53, "vertices": 2286, "boundary": 0, "isolated": 0, "clamped": 0,
                    "max_move": info["max_move"]}
    assert out["vertices"].dtype == np.float32 and np.isfinite(out["vertices"]).all()


def test_adjacency_of_a_closed_mesh_and_of_odd_faces():
    v, c, f = S.sphere()
    adj = S.adjacency(f, len(v))
    assert not adj["boundary"].any() and not adj["isolated"].any() and int(adj["start"][-1]) == 6 * len(f)
    assert adj["degree"].sum() * 2 == 6 * len(f) and (adj["degree"] * 2 == np.diff(adj["start"])).all()     # every edge twice
    v, c, f = S.repeated_corners()
    adj = S.adjacency(f, len(v))
    n = [S.used(adj)[a:b].tolist() for a, b in zip(np.cumsum(adj["degree"]) - adj["degree"], np.cumsum(adj["degree"]))]
    # {1,3}: (1,1,3) gives it twice, (3,1,1) twice more; {4,5} twice from (4,5,4); 6 and 11 are isolated; {0,1}, {1,2} twice
    # from the duplicate face, {0,2} three times; {0,3}, {2,3} once: 0, 2, 3 are boundary vertices
    assert n[6] == [] and n[11] == [] and adj["isolated"].tolist() == [i in (6, 11) for i in range(12)]
    assert n[1] == [0, 2, 3] and n[4] == [5] and n[5] == [4] and not adj["boundary"][[1, 4, 5]].any()
    assert n[0] == [3] and n[2] == [3] and n[3] == [0, 2] and adj["boundary"][[0, 2, 3]].all()
    assert n[8] == [7, 10] and n[9] == [7, 10] and n[7] == [8, 9] and n[10] == [8, 9]                # {8,9} is interior: skipped
    assert int(adj["start"][-1]) == 2 * (3 + 2 + 2 + 0 + 3 + 3 + 3 + 3 + 0 + 2)
    far = np.concatenate([f, [[0, 1, 12], [-1, 2, 3]]]).astype(np.int32)                            # invalid faces are skipped
    again = S.adjacency(far, len(v))
    assert all(np.array_equal(adj[k], again[k]) for k in adj)


# ---------------------------------------------------------------------------------------------------------- the boundary
def test_open_patch_relaxes_along_its_border_and_in_its_plane():
    nx, ny = 9, 7
    v, c, f = S.grid_patch(nx, ny)
    out, info = S.smooth(v, c, f, 10)
    p = out["vertices"].reshape(ny, nx, 3)
    assert info["boundary"] == 2 * (nx + ny) - 4 and info["isolated"] == 0
    assert (p[..., 2] == np.float32(2.5)).all()                          # the plane: the mean of equal numbers is that number
    # one step: a border vertex between two others reads only those two, so it stays on its line and moves along it; a corner
    # has two boundary neighbours, one along either line, and moves towards their mean (later steps carry that on along the border)
    adj = S.adjacency(f, len(v))
    first = S.step(v, adj, 0.5).reshape(ny, nx, 3)
    q = v.reshape(ny, nx, 3)
    assert (first[0, 1:-1, 1] == 0).all() and (first[-1, 1:-1, 1] == ny - 1).all()
    assert (first[1:-1, 0, 0] == 0).all() and (first[1:-1, -1, 0] == nx - 1).all()
    assert (first[0, 1:-1, 0] != q[0, 1:-1, 0]).any() and (first[1:-1, 0, 1] != q[1:-1, 0, 1]).any()
    want = q[0, 1:-1, 0].astype(np.float64) + 0.5 * ((q[0, :-2, 0].astype(np.float64) + q[0, 2:, 0]) / 2 - q[0, 1:-1, 0])
    assert np.array_equal(first[0, 1:-1, 0], want.astype(np.float32))    # not pulled by the inner neighbours
    q = q.astype(np.float64)
    want = q[0, 0] + 0.5 * ((q[0, 1] + q[1, 0]) / 2 - q[0, 0])
    assert np.array_equal(first[0, 0], want.astype(np.float32)) and first[0, 0, 0] > 0 and first[0, 0, 1] > 0
    sv, sc, sf = S.grid_patch(7, 7, jitter=0.0)                          # a regular square patch
    square, _ = S.smooth(sv, sc, sf, 10)
    s = square["vertices"].reshape(7, 7, 3)
    assert s[0, 0, 0] == s[0, 0, 1] and s[-1, -1, 0] == s[-1, -1, 1]     # the corners move along the diagonals
    assert np.isclose(6 - s[0, -1, 0], s[0, -1, 1]) and np.isclose(s[-1, 0, 0], 6 - s[-1, 0, 1]) and 0 < s[0, 0, 0] < 1


# ------------------------------------------------------------------------------------------------------------- the limit
@pytest.mark.parametrize("D", [0.08, 0.3])
def test_max_move_holds_and_counts(D):
    v, c, f = S.noisy_sphere()
    free, finfo = S.smooth(v, c, f, 10)
    out, info = S.smooth(v, c, f, 10, max_move=D)
    d0 = free["vertices"].astype(np.float64) - v
    n2 = (d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]) + d0[:, 2] * d0[:, 2]
    assert info["clamped"] == int((n2 > D * D).sum()) and 0 < info["clamped"] < len(v)
    assert info["max_move"] == finfo["max_move"] == float(np.sqrt(n2.max()))                    # taken before the clamp
    moved = np.linalg.norm(out["vertices"].astype(np.float64) - v, axis=1)
    ulp = float(np.spacing(np.float32(np.abs(v).max())))
    assert moved.max() <= D + ulp
    same = n2 <= D * D
    assert np.array_equal(out["vertices"][same].view(np.uint32), free["vertices"][same].view(np.uint32))
    assert (moved[~same] > D - 3 * ulp).all()


# ------------------------------------------------------------------------------------------------------- public interface
def test_no_cpu_path_and_argument_checks():
    v, col, f = (torch.from_numpy(np.ascontiguousarray(a)) for a in S.grid_patch())
    m = {"vertices": v, "colors": col, "faces": f}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.smooth_mesh(m, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.mesh_adjacency(f, len(v))
    for bad in (0, -1, 1001, 2.0, "3", None, True, float("nan")):
        with pytest.raises(ValueError, match="iterations must be an int in 1..1000"):
            mesh.smooth_mesh(m, bad)
    for bad in (0.0, -0.5, 1.5, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="lam must be finite and in"):
            mesh.smooth_mesh(m, 3, lam=bad)
    for bad in (0.1, -1.5, float("nan"), -float("inf"), "x", None):
        with pytest.raises(ValueError, match="mu must be finite and in"):
            mesh.smooth_mesh(m, 3, mu=bad)
    for bad in (-0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="max_move must be finite and in"):
            mesh.smooth_mesh(m, 3, max_move=bad)
    assert mesh.check_smooth(1, 1.0, -1.0, 0.0) == (1, 1.0, -1.0, 0.0) and mesh.check_smooth(np.int64(1000), 0.25, 0, 2) == (1000, 0.25, 0.0, 2.0)
    with pytest.raises(ValueError, match="vertices must be"):
        mesh.smooth_mesh(dict(m, vertices=v.double()), 3)
    with pytest.raises(ValueError, match="colors must be"):
        mesh.smooth_mesh(dict(m, colors=col[:5]), 3)
    with pytest.raises(ValueError, match="faces must be an int32"):
        mesh.smooth_mesh(dict(m, faces=f.long()), 3)
    for bad in (f.long(), f[:, :2], f.numpy()):
        with pytest.raises(ValueError, match="faces must be an int32"):
            mesh.mesh_adjacency(bad, len(v))
    with pytest.raises(ValueError, match="iterations must be"):
        mesh.mesh_scan("nowhere", "nowhere", "nowhere.ply", 1.0, smooth=-2)
    with pytest.raises(ValueError, match="lam must be"):
        mesh.mesh_scan("nowhere", "nowhere", "nowhere.ply", 1.0, smooth=2, smooth_lambda=2.0)
    with pytest.raises(ValueError, match="mu must be"):
        mesh.clean_file("nowhere.ply", "nowhere.ply", smooth=2, smooth_mu=0.5)
    with pytest.raises(ValueError, match="max_move must be"):
        mesh.clean_file("nowhere.ply", "nowhere.ply", smooth=2, smooth_max_move=-1.0)
    assert mesh._check_smooth(0, 9.0, 9.0, -9.0, "x") is None and mesh._check_smooth(None, 0.5, -0.53, 0.0, "x") is None
    assert (mesh.MAX_SMOOTH, mesh.ADJ_SMALL, mesh.ADJ_BOUNDARY, mesh.ADJ_ISOLATED) == (1000, 64, 1, 2)


def test_header_signatures_and_makefile():
    header = open(os.path.join(ROOT, "include", "cds_mvsnet_hip.h")).read()
    for name, nargs in (("cds_mesh_adj_count", 5), ("cds_mesh_adj_fill", 8), ("cds_mesh_adj_finish", 7),
                        ("cds_mesh_smooth_step_f32", 8), ("cds_mesh_smooth_limit_f32", 7)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\);", header, re.M | re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert _lib.SIGNATURES["cds_mesh_adj_small"] == [] and re.search(r"^int\s+cds_mesh_adj_small\s*\(void\);", header, re.M)
    for name, value in (("CDS_MESH_ADJ_SMALL", mesh.ADJ_SMALL), ("CDS_MESH_ADJ_BOUNDARY", mesh.ADJ_BOUNDARY),
                        ("CDS_MESH_ADJ_ISOLATED", mesh.ADJ_ISOLATED)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", header), name
    assert "csrc/mesh_smooth.hip; DESIGN 1.15" in header
    makefile = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", makefile, re.M).group(1).split()
    assert "mesh_smooth.hip" in srcs and os.path.exists(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "mesh_smooth.hip"))
    source = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "mesh_smooth.hip")).read()
    assert "asm" not in source
    adds = re.findall(r"atomicAdd\(([^;]*);", source)
    assert adds and all(re.match(r"&(count|cursor)\[\w+\], 1\)", a) for a in adds), adds      # int32 counters only
    assert not re.search(r"atomic(?!Add\()\w*\(", source)                                       # and no other atomic


def test_options_and_printed_line(capsys):
    ap = argparse.ArgumentParser()
    mesh.add_mesh_args(ap)
    args = ap.parse_args(["--mesh_voxel", "2"])
    assert (args.mesh_smooth, args.mesh_smooth_lambda, args.mesh_smooth_mu, args.mesh_smooth_max_move) == (None, None, None, None)
    assert mesh.smooth_args(args) == (0, 0.5, -0.53, 0.0)
    args = ap.parse_args(["--mesh_voxel", "2", "--mesh_smooth", "7", "--mesh_smooth_lambda", "0.4", "--mesh_smooth_mu", "-0.42",
                          "--mesh_smooth_max_move", "1.5"])
    assert mesh.smooth_args(args) == (7, 0.4, -0.42, 1.5)
    base = ["--testpath", "x", "--testlist", "x", "--outdir", "x"]
    got = infer.parse_args(base + ["--fuse", "--mesh_voxel", "2", "--mesh_smooth", "5", "--mesh_smooth_mu", "0"])
    assert mesh.smooth_args(got) == (5, 0.5, 0.0, 0.0)
    assert infer.parse_args(base + ["--fuse", "--mesh_voxel", "2"]).mesh_smooth is None
    bad_values = (["--mesh_smooth", "0"], ["--mesh_smooth", "-1"], ["--mesh_smooth", "1001"], ["--mesh_smooth", "2.5"],
                  ["--mesh_smooth", "3", "--mesh_smooth_lambda", "0"], ["--mesh_smooth", "3", "--mesh_smooth_lambda", "1.1"],
                  ["--mesh_smooth", "3", "--mesh_smooth_lambda", "nan"], ["--mesh_smooth", "3", "--mesh_smooth_mu", "0.1"],
                  ["--mesh_smooth", "3", "--mesh_smooth_mu", "-1.1"], ["--mesh_smooth", "3", "--mesh_smooth_mu", "nan"],
                  ["--mesh_smooth", "3", "--mesh_smooth_max_move", "-1"], ["--mesh_smooth", "3", "--mesh_smooth_max_move", "inf"],
                  ["--mesh_smooth_lambda", "0.5"], ["--mesh_smooth_mu", "-0.5"], ["--mesh_smooth_max_move", "1"])   # without --mesh_smooth
    for extra in bad_values:
        with pytest.raises(SystemExit):
            infer.parse_args(base + ["--fuse", "--mesh_voxel", "2"] + extra)
        with pytest.raises(SystemExit):
            mesh.main(["--outdir", "x", "--testlist", "x", "--from_mesh", "y"] + extra)
    for extra in (["--mesh_smooth", "3"], ["--mesh_smooth_lambda", "0.5"], ["--mesh_smooth_mu", "-0.5"],
                  ["--mesh_smooth_max_move", "1"]):                                               # no mesh to smooth
        with pytest.raises(SystemExit):
            infer.parse_args(base + ["--fuse"] + extra)
        with pytest.raises(SystemExit):
            mesh.main(["--outdir", "x", "--testlist", "x"] + extra)
    capsys.readouterr()
    old = {"vertices": 7, "faces": 5, "blocks": 3}
    assert mesh.format_mesh(old) == "7 vertices, 5 faces, 3 blocks"                                # the line of a run without the option
    sm = {"iterations": 5, "lam": 0.5, "mu": -0.53, "vertices": 7, "boundary": 4, "isolated": 1, "clamped": 0, "max_move": 0.25,
          "limit": 0.0}
    line = mesh.format_mesh(dict(old, smooth=sm))
    assert line == ("7 vertices, 5 faces, 3 blocks; smoothed 5 iterations (lambda 0.5, mu -0.53): 4 boundary, 1 isolated vertices, "
                    "largest move 0.25")
    line = mesh.format_mesh(dict(old, smooth=dict(sm, clamped=2, limit=0.125)))
    assert line.endswith("largest move 0.25, 2 clamped to 0.125")
    clean = {"components": (4, 1), "vertices": (40, 20), "faces": (60, 30), "largest": 30, "rounds": 2}
    simp = {"vertices": (20, 7), "faces": (30, 5), "clusters": 9, "collapsed": 22, "duplicates": 3, "fallback": 1}
    allp = mesh.format_mesh(dict(old, clean=clean, simplify=simp, smooth=sm))
    assert allp.index("removed 3 of 4 components") < allp.index("smoothed 5 iterations") < allp.index("simplified 20 -> 7")
    assert mesh.format_mesh(dict(old, clean=clean, simplify=simp)) == allp.replace(
        "; smoothed 5 iterations (lambda 0.5, mu -0.53): 4 boundary, 1 isolated vertices, largest move 0.25", "")


def test_off_by_default_nothing_of_it_runs(tmp_path, monkeypatch):
    """_finish without a smoothing tuple never reaches smooth_mesh, and writes the mesh it was given; with one, and with the
    other steps, the order is clean, smooth, simplify.  The steps are replaced: this is the CPU-reachable part only."""
    v, c, f = S.grid_patch()
    m = {"vertices": torch.from_numpy(v), "colors": torch.from_numpy(c), "faces": torch.from_numpy(f)}
    calls = []

    def no_smooth(*a, **k):
        raise AssertionError("smooth_mesh ran without iterations")
    monkeypatch.setattr(mesh, "smooth_mesh", no_smooth)
    path = str(tmp_path / "plain_mesh.ply")
    info = mesh._finish(m, path, None, None, 0.0, "quadric", 0.0, None)
    assert sorted(info) == ["faces", "mesh", "vertices"] and info["mesh"] is m
    got = mesh.read_mesh_ply(path)
    assert all(np.array_equal(a, b) for a, b in zip(got, (v, c, f)))
    monkeypatch.setattr(mesh, "clean_mesh", lambda mm, *a: (calls.append(("clean", a)), (mm, {"c": 1}))[1])
    monkeypatch.setattr(mesh, "simplify_mesh", lambda mm, *a: (calls.append(("simplify", a)), (mm, {"s": 1}))[1])
    info = mesh._finish(m, path, (3, 0), None, 2.0, "mean", 0.0, None)
    assert calls == [("clean", (3, 0)), ("simplify", (2.0, "mean"))] and "smooth" not in info
    del calls[:]
    monkeypatch.setattr(mesh, "smooth_mesh", lambda mm, *a: (calls.append(("smooth", a)), (mm, {"iterations": a[0]}))[1])
    info = mesh._finish(m, path, (3, 0), (5, 0.5, -0.53, 0.25), 2.0, "mean", 0.0, None)
    assert calls == [("clean", (3, 0)), ("smooth", (5, 0.5, -0.53, 0.25)), ("simplify", (2.0, "mean"))]
    assert info["smooth"] == {"iterations": 5, "limit": 0.25} and info["clean"] == {"c": 1} and info["simplify"] == {"s": 1}
    # mesh_scan and clean_file turn 0 iterations into "off" before anything else happens
    seen = {}
    monkeypatch.setattr(mesh, "_finish", lambda mm, ply, clean, smooth, *a: seen.update(clean=clean, smooth=smooth) or {})
    monkeypatch.setattr(mesh, "read_mesh_ply", lambda path: (v, c, f))
    mesh.clean_file("a.ply", "b.ply", device="cpu")
    assert seen == {"clean": (0, 0), "smooth": None}
    mesh.clean_file("a.ply", "b.ply", device="cpu", smooth=4, smooth_max_move=0.5)
    assert seen == {"clean": None, "smooth": (4, 0.5, -0.53, 0.5)}                                # smoothing alone: no clean-up
    mesh.clean_file("a.ply", "b.ply", min_component=2, device="cpu", smooth=4)
    assert seen == {"clean": (2, 0), "smooth": (4, 0.5, -0.53, 0.0)}
