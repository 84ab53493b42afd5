"""The numpy restatement of the hole-filling rule (mesh_fill_ref.py) held to closed forms and to a second border
finder, and the parts of the stage that run without a GPU: the options, the printed line, the order of the finishing chain and
the list of sources."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import mesh_fill_ref as R
from cds_mvsnet_amd import _lib, infer, mesh
from cds_mvsnet_amd.mesh import MAX_FILL_EDGES, check_fill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _closed(faces, nv):
    b = R.borders(faces, nv)
    return b["border_edges"] == 0 and not b["regular"].any() and (b["next"] == -1).all()


def test_tetrahedron_without_a_face_closes_with_one_face():
    assert R.MAX_EDGES == MAX_FILL_EDGES == 4096
    v, c, f = R.open_tetrahedron()
    assert R.borders(f, 4)["border_edges"] == 3 and R.loops(f, 4)[0] == [[1, 3, 2]]
    out, info = R.fill(v, c, f, 3)
    assert info == {"max_edges": 3, "loops": 1, "largest": 3, "border_edges": (3, 0), "vertices": (4, 4), "faces": (3, 4)}
    assert np.array_equal(out["faces"][:3], f) and out["faces"][3].tolist() == [1, 2, 3]          # (v0, v2, v1) of the loop 1, 3, 2
    assert np.array_equal(out["vertices"], v) and np.array_equal(out["colors"], c)
    assert _closed(out["faces"], 4) and R.signed_volume(out["vertices"], out["faces"]) == 1.0 / 6.0


def test_cube_without_a_side_gains_its_centre_and_volume_one():
    v, c, f = R.cube()
    assert len(f) == 10 and R.signed_volume(*R.cube(open_side=False)[::2]) == 1.0
    side = R.loops(f, 8)[0]
    assert side == [[1, 5, 7, 3]]
    for max_edges in (4, 64, MAX_FILL_EDGES):
        out, info = R.fill(v, c, f, max_edges)
        assert info == {"max_edges": max_edges, "loops": 1, "largest": 4, "border_edges": (4, 0), "vertices": (8, 9), "faces": (10, 14)}
        assert out["vertices"][8].tolist() == [1.0, 0.5, 0.5] and np.array_equal(out["vertices"][:8], v)
        assert out["faces"][10:].tolist() == [[5, 1, 8], [7, 5, 8], [3, 7, 8], [1, 3, 8]]
        want = [(2 * int(c[[1, 5, 7, 3], k].sum()) + 4) // 8 for k in range(3)]
        assert out["colors"][8].tolist() == want
        assert _closed(out["faces"], 9) and R.signed_volume(out["vertices"], out["faces"]) == 1.0
    out, info = R.fill(v, c, f, 3)                                       # the cap: a loop of 4 stays at max_edges 3
    assert info["loops"] == 0 and info["border_edges"] == (4, 4) and np.array_equal(out["faces"], f) and len(out["vertices"]) == 8


def test_lone_triangle_becomes_a_pillow():
    out, info = R.fill(*R.lone_triangle(), 3)
    assert out["faces"].tolist() == [[0, 1, 2], [0, 2, 1]] and info["border_edges"] == (3, 0) and _closed(out["faces"], 3)


@pytest.mark.parametrize("seed", range(6))
def test_a_second_border_finder_agrees(seed):
    """np.unique over sorted undirected keys against the dict of edges: the count and the directed border half-edges, on random
    face soups (edges held once, twice either way, three times and more, repeated corners) and on punched grids."""
    for v, c, f in (R.random_faces(40 + 7 * seed, 90 + 30 * seed, seed), R.random_punched_grid(seed)):
        nv = len(v)
        count, directed = R.border_count_by_unique(f, nv)
        b = R.borders(f, nv)
        assert b["border_edges"] == count > 0
        leave = np.bincount(directed[:, 0], minlength=nv)
        enter = np.bincount(directed[:, 1], minlength=nv)
        regular = (leave == 1) & (enter == 1)
        assert np.array_equal(b["regular"], regular)
        nxt = np.full(nv, -1, np.int32)
        one = regular[directed[:, 0]]
        nxt[directed[one, 0]] = directed[one, 1]
        assert np.array_equal(b["next"], nxt)
        out, info = R.fill(v, c, f, 16)                                  # and what is filled is no border afterwards
        after = R.border_count_by_unique(out["faces"], len(out["vertices"]))[0]
        assert info["border_edges"] == (count, after) and np.array_equal(out["faces"][:len(f)], f)


def test_the_cap_and_what_stays_open():
    for n in (3, 4, 5, 8, 63, 64, 65):
        v, c, f = R.grid_with_hole(n)
        found = sorted(len(p) for p in R.loops(f, len(v))[0])
        assert found == sorted([n, 48])
        out, info = R.fill(v, c, f, 47)
        assert info["loops"] == (1 if n <= 47 else 0) and info["border_edges"] == (48 + n, 48 + (0 if n <= 47 else n))
        out, info = R.fill(v, c, f, 64)
        assert info["loops"] == (2 if n <= 64 else 1) and info["largest"] == max(48, n if n <= 64 else 0)
    for name, builder, stays in (("bow tie", R.bow_tie, 8), ("fin", R.fin, 2), ("flipped", R.flipped, 0)):
        v, c, f = builder()
        out, info = R.fill(v, c, f, 23)                                  # below the rim of the 6 x 6 grid
        before, after = info["border_edges"]
        assert after == 24 + stays, name
    v, c, f = R.bow_tie()
    assert not R.borders(f, len(v))["regular"][3 * 7 + 3]
    v, c, f = R.with_degenerate_faces()
    out, info = R.fill(v, c, f, 8)
    assert info["loops"] == 1 and info["largest"] == 5 and np.array_equal(out["faces"][:len(f)], f)


def test_new_faces_are_oriented_as_the_surface():
    """The grid faces +z; so does every face of every fan, and the new vertex lies in its plane."""
    v, c, f = R.grid_with_hole(9)
    out, info = R.fill(v, c, f, 47)                                      # below the grid's own rim, whose cap would face -z
    p = out["vertices"].astype(np.float64)[out["faces"]]
    normals = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (normals[:, 2] > 0).all() and (normals[:, :2] == 0).all() and (out["vertices"][len(v):, 2] == 0.5).all()
    assert info["loops"] == 1 and abs(normals[:, 2].sum() / 2.0 - 144.0) < 1e-9                  # the grid's area is whole again


def test_options_and_printed_line():
    assert check_fill(3) == 3 and check_fill(np.int64(4096)) == 4096
    for bad in (2, 4097, 3.5, True, None, "7", 0, -1):
        with pytest.raises(ValueError, match="max_edges must be an int in 3..4096"):
            check_fill(bad)
        with pytest.raises(ValueError, match="max_edges must be an int in 3..4096"):
            mesh.fill_holes({}, bad)                                     # before the mesh is looked at
    ap = argparse.ArgumentParser()
    mesh.add_mesh_args(ap)
    assert ap.parse_args(["--mesh_voxel", "2"]).mesh_fill_holes is None
    assert ap.parse_args(["--mesh_voxel", "2", "--mesh_fill_holes", "16"]).mesh_fill_holes == 16
    base = ["--testpath", "x", "--testlist", "x", "--outdir", "x"]
    assert infer.parse_args(base + ["--fuse", "--mesh_voxel", "2", "--mesh_fill_holes", "16"]).mesh_fill_holes == 16
    assert infer.parse_args(base + ["--fuse", "--mesh_voxel", "2"]).mesh_fill_holes is None
    for extra in (["--mesh_fill_holes", "2"], ["--mesh_fill_holes", "0"], ["--mesh_fill_holes", "4097"], ["--mesh_fill_holes", "3.5"],
                  ["--mesh_fill_holes", "-3"]):
        with pytest.raises(SystemExit):
            infer.parse_args(base + ["--fuse", "--mesh_voxel", "2"] + extra)
        with pytest.raises(SystemExit):
            mesh.main(["--outdir", "x", "--testlist", "x", "--from_mesh", "y"] + extra)
    with pytest.raises(SystemExit):                                      # no mesh to fill
        infer.parse_args(base + ["--fuse", "--mesh_fill_holes", "16"])
    with pytest.raises(SystemExit):
        mesh.main(["--outdir", "x", "--testlist", "x", "--mesh_fill_holes", "16"])
    old = {"vertices": 7, "faces": 5, "blocks": 3}
    assert mesh.format_mesh(old) == "7 vertices, 5 faces, 3 blocks"
    fill = {"max_edges": 16, "loops": 4, "largest": 9, "border_edges": (120, 98), "vertices": (5, 7), "faces": (1, 5)}
    assert mesh.format_mesh(dict(old, fill=fill)) == ("7 vertices, 5 faces, 3 blocks; filled 4 holes of at most 16 edges (the largest "
                                                     "has 9), border edges 120 -> 98")
    clean = {"components": (4, 1), "vertices": (40, 20), "faces": (60, 30), "largest": 30, "rounds": 2}
    sm = {"iterations": 5, "lam": 0.5, "mu": -0.53, "vertices": 7, "boundary": 4, "isolated": 1, "clamped": 0, "max_move": 0.25, "limit": 0.0}
    line = mesh.format_mesh(dict(old, clean=clean, fill=fill, smooth=sm))
    assert line.index("removed 3 of 4 components") < line.index("filled 4 holes") < line.index("smoothed 5 iterations")


def test_off_by_default_and_the_order_of_the_chain(tmp_path, monkeypatch):
    """_finish without a fill never reaches fill_holes and writes the mesh it was given; with one, the order is clean, fill, smooth,
    simplify.  The steps are replaced: this is the CPU-reachable part only."""
    v, c, f = R.grid_with_hole(5, 6)
    m = {"vertices": torch.from_numpy(v), "colors": torch.from_numpy(c), "faces": torch.from_numpy(f)}
    calls = []

    def no_fill(*a, **k):
        raise AssertionError("fill_holes ran without --mesh_fill_holes")
    monkeypatch.setattr(mesh, "fill_holes", no_fill)
    path = str(tmp_path / "plain_mesh.ply")
    for args in ((), (0,)):
        info = mesh._finish(m, path, None, None, 0.0, "quadric", 0.0, None, *args)
        assert sorted(info) == ["faces", "mesh", "vertices"] and info["mesh"] is m
        assert all(np.array_equal(a, b) for a, b in zip(mesh.read_mesh_ply(path), (v, c, f)))
    monkeypatch.setattr(mesh, "clean_mesh", lambda mm, *a: (calls.append(("clean", a)), (mm, {"c": 1}))[1])
    monkeypatch.setattr(mesh, "smooth_mesh", lambda mm, *a: (calls.append(("smooth", a)), (mm, {"iterations": a[0]}))[1])
    monkeypatch.setattr(mesh, "simplify_mesh", lambda mm, *a: (calls.append(("simplify", a)), (mm, {"s": 1}))[1])
    monkeypatch.setattr(mesh, "fill_holes", lambda mm, *a: (calls.append(("fill", a)), (mm, {"loops": 1}))[1])
    info = mesh._finish(m, path, (3, 0), (5, 0.5, -0.53, 0.25), 2.0, "mean", 0.0, None, 16)
    assert calls == [("clean", (3, 0)), ("fill", (16,)), ("smooth", (5, 0.5, -0.53, 0.25)), ("simplify", (2.0, "mean"))]
    assert info["fill"] == {"loops": 1} and info["clean"] == {"c": 1}
    # mesh_scan and clean_file turn 0 into "off"; a fill alone skips the clean-up as smoothing alone does
    seen = {}
    monkeypatch.setattr(mesh, "_finish", lambda mm, ply, clean, smooth, *a: seen.update(clean=clean, smooth=smooth, fill=a[-1]) or {})
    monkeypatch.setattr(mesh, "read_mesh_ply", lambda path: (v, c, f))
    mesh.clean_file("a.ply", "b.ply", device="cpu")
    assert seen == {"clean": (0, 0), "smooth": None, "fill": 0}
    mesh.clean_file("a.ply", "b.ply", device="cpu", fill_holes=16)
    assert seen == {"clean": None, "smooth": None, "fill": 16}
    mesh.clean_file("a.ply", "b.ply", device="cpu", fill_holes=16, min_component=2, smooth=4)
    assert seen == {"clean": (2, 0), "smooth": (4, 0.5, -0.53, 0.0), "fill": 16}
    for bad in (2, 4097, 3.5, True):
        with pytest.raises(ValueError, match="max_edges must be an int"):
            mesh.clean_file("a.ply", "b.ply", device="cpu", fill_holes=bad)
        with pytest.raises(ValueError, match="max_edges must be an int"):
            mesh.mesh_scan("nowhere", "nowhere", "nowhere.ply", 1.0, fill_holes=bad)


def test_the_source_is_listed_and_bound():
    makefile = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", makefile, re.M).group(1).split()
    assert "mesh_fill.hip" in srcs and os.path.exists(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "mesh_fill.hip"))
    source = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "mesh_fill.hip")).read()
    assert "asm" not in source
    adds = re.findall(r"atomicAdd\(([^;]*);", source)
    assert adds and all(re.match(r"&(out|in)\[\w+\], 1\)", a) for a in adds), adds                # int32 counters only
    assert not re.search(r"atomic(?!Add\()\w*\(", source)                                          # and no other atomic
    header = open(os.path.join(ROOT, "include", "cds_mvsnet_hip.h")).read()
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("cds_mesh_fill_"))
    assert names == ["cds_mesh_fill_borders", "cds_mesh_fill_double", "cds_mesh_fill_emit", "cds_mesh_fill_init", "cds_mesh_fill_keys",
                     "cds_mesh_fill_max_edges", "cds_mesh_fill_walk"]
    for name in names:
        assert re.search(r"^int " + name + r"\(", header, re.M) and re.search(r'^extern "C" int ' + name + r"\(", source, re.M), name
    assert f"#define CDS_MESH_FILL_MAX_EDGES {MAX_FILL_EDGES}\n" in header
