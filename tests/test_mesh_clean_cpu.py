"""The numpy restatement of the component rule (mesh_clean_ref.py) against things known otherwise: meshes whose
components, counts and labels are known by construction, a second algorithm (label propagation to a fixed point), and the
parts of the public interface that need no GPU: argument checks, the command-line options and the printed line."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_ref as M
from cds_mvsnet_amd import _lib, infer, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _propagate(faces, nv):
    """Rules 1 and 2 by another way: every vertex takes the smallest label of a face it is in, until nothing changes."""
    lab = np.arange(nv, dtype=np.int64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    while True:
        low = lab[faces].min(1)
        new = lab.copy()
        for k in range(3):
            np.minimum.at(new, faces[:, k], low)
        if np.array_equal(new, lab):
            return lab.astype(np.int32)
        lab = new


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                                        b.view(np.uint32) if b.dtype == np.float32 else b)


def test_sphere_is_one_component():
    m = M.analytic_case("sphere")[1]
    v, f = m["vertices"], m["faces"]
    assert f.shape == (4568, 3) and v.shape == (2286, 3)
    c = C.components(f, len(v))
    assert (c["label"] == 0).all() and c["components"].tolist() == [0] and c["faces"].tolist() == [4568]
    assert c["label"].dtype == np.int32 and c["components"].dtype == np.int32 and c["faces"].dtype == np.int64


def test_sphere_with_two_tetrahedra():
    v, col, f = C.sphere_with_debris()
    sphere = M.analytic_case("sphere")[1]
    c = C.components(f, len(v))
    assert c["components"].tolist() == [0, 2286, 2290] and c["faces"].tolist() == [4568, 4, 4]
    assert (c["label"][:2286] == 0).all() and (c["label"][2286:2290] == 2286).all() and (c["label"][2290:] == 2290).all()
    assert np.array_equal(c["label"], _propagate(f, len(v)))
    out, info = C.clean(v, col, f, min_faces=5)                          # the sphere exactly
    assert _same(out["vertices"], sphere["vertices"]) and _same(out["colors"], sphere["colors"]) and _same(out["faces"], sphere["faces"])
    assert info == {"components": (3, 1), "vertices": (2294, 2286), "faces": (4576, 4568), "largest": 4568}
    out, info = C.clean(v, col, f, keep_largest=2)                       # the sphere and the tetrahedron with the lower label
    assert _same(out["vertices"], v[:2290]) and _same(out["colors"], col[:2290]) and _same(out["faces"], f[:4572])
    assert info["components"] == (3, 2) and info["faces"] == (4576, 4572)
    out, _ = C.clean(v, col, f, min_faces=4, keep_largest=1)             # both conditions: the sphere
    assert _same(out["faces"], sphere["faces"])
    out, _ = C.clean(v, col, f, min_faces=5, keep_largest=3)
    assert _same(out["faces"], sphere["faces"])
    out, info = C.clean(v, col, f, min_faces=4569)
    assert out["vertices"].shape == (0, 3) and out["colors"].shape == (0, 3) and out["faces"].shape == (0, 3)
    assert info["components"] == (3, 0) and info["vertices"] == (2294, 0)
    # dropping the sphere renumbers the tetrahedra
    only = np.concatenate([f[4568:], f[:4568]])                          # the same mesh, the tetrahedra's faces first
    out, _ = C.clean(v, col, only, keep_largest=1)
    assert _same(out["faces"], sphere["faces"])
    keep = C.select(np.array([4568, 4, 4]), 0, 0)
    assert keep.tolist() == [True, True, True]


def test_two_fans_that_share_a_vertex_are_one_component():
    v, col, f = C.two_fans()
    c = C.components(f, len(v))
    assert c["components"].tolist() == [0] and c["faces"].tolist() == [6] and (c["label"] == 0).all()
    tp = M.topology(f, len(v))                                           # no edge joins the fans: edge adjacency would give two
    edges = {tuple(sorted(e)) for t in f.tolist() for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
    assert tp["edges"] == len(edges) and not any(a in (0, 1, 2, 4) and b in (5, 6, 7, 8) for a, b in edges)
    out, info = C.clean(v, col, f, min_faces=6)
    assert _same(out["faces"], f) and _same(out["vertices"], v)
    assert C.clean(v, col, f, min_faces=7)[0]["faces"].shape == (0, 3)


def test_degenerate_duplicate_and_unreferenced():
    v, col, f = C.odd_faces()
    c = C.components(f, len(v))
    assert c["label"].tolist() == [0, 1, 2, 2, 1, 2, 1, 1, 1, 9]
    assert c["components"].tolist() == [0, 1, 2, 9] and c["faces"].tolist() == [0, 3, 2, 0]      # the duplicate counts twice
    assert np.array_equal(c["label"], _propagate(f, len(v)))
    out, info = C.clean(v, col, f)                                       # the defaults drop only the vertices in no face
    used = [1, 2, 3, 4, 5, 6, 7, 8]
    assert _same(out["vertices"], v[used]) and _same(out["colors"], col[used]) and _same(out["faces"], f - 1)
    assert info == {"components": (4, 2), "vertices": (10, 8), "faces": (5, 5), "largest": 3}
    out, info = C.clean(v, col, f, min_faces=3)
    assert out["faces"].tolist() == [[0, 0, 1], [1, 2, 3], [1, 3, 4]] and _same(out["vertices"], v[[1, 4, 6, 7, 8]])
    out, info = C.clean(v, col, f, keep_largest=3)                       # rank: 1 (3 faces), 2 (2), 0 (0 faces, before 9)
    assert info["components"] == (4, 2) and info["faces"] == (5, 5)
    out, info = C.clean(v, col, f, keep_largest=1)
    assert info["faces"] == (5, 3)


@pytest.mark.parametrize("min_faces", [0, 1])
def test_identity_when_every_vertex_is_in_a_face(min_faces):
    for v, col, f in (C.sphere_with_debris(), C.two_fans(), C.isolated_triangles(65)):
        out, info = C.clean(v, col, f, min_faces=min_faces)
        assert _same(out["vertices"], v) and _same(out["colors"], col) and _same(out["faces"], f)
        assert info["components"][0] == info["components"][1] and info["vertices"] == (len(v), len(v))


def test_ties_in_keep_largest_go_to_the_lower_label():
    assert C.select(np.array([2, 5, 5, 1, 5]), 0, 2).tolist() == [False, True, True, False, False]
    assert C.select(np.array([2, 5, 5, 1, 5]), 0, 4).tolist() == [True, True, True, False, True]
    assert C.select(np.array([2, 5, 5, 1, 5]), 3, 4).tolist() == [False, True, True, False, True]
    assert C.select(np.array([2, 5, 5, 1, 5]), 2, 9).tolist() == [True, True, True, False, True]
    got = mesh.select_components(torch.tensor([2, 5, 5, 1, 5]), 0, 2)    # the torch statement the GPU path uses, here on the host
    assert got.tolist() == [False, True, True, False, False]
    rng = np.random.default_rng(5)
    for _ in range(20):
        counts = rng.integers(0, 4, 30)
        for mf, k in ((0, 0), (2, 0), (0, 7), (1, 12), (3, 3)):
            assert mesh.select_components(torch.from_numpy(counts), mf, k).tolist() == C.select(counts, mf, k).tolist()


@pytest.mark.parametrize("n_faces", [300, 1000, 3000])
def test_random_graphs_two_ways(n_faces):
    f = C.random_faces(2000, n_faces, seed=n_faces)
    repeated = int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum())
    assert n_faces < 3000 or repeated > 0                               # faces with a repeated index occur (4.5 expected at 3000)
    c = C.components(f, 2000)
    assert np.array_equal(c["label"], _propagate(f, 2000))
    assert c["faces"].sum() == n_faces and (c["label"] <= np.arange(2000)).all()
    print(f"F = {n_faces}: {len(c['components'])} components, the largest has {c['faces'].max()} faces")


def test_strips_are_one_component():
    for order in ("ascending", "descending", "random"):
        f = C.strip(1 << 10, order, seed=1)
        assert (C.labels(f, 1 << 10) == 0).all()
    f, nv = C.strip_and_triangles(1 << 10, 100)
    c = C.components(f, nv)
    assert len(f) == (1 << 10) - 2 + 100 and c["faces"].tolist() == [(1 << 10) - 2] + [1] * 100
    assert (np.diff(np.nonzero(f[:, 0] >= 1 << 10)[0]) > 1).all()        # the triangles are spread over the face list


# ------------------------------------------------------------------------------------------------------- public interface
def test_no_cpu_path_and_argument_checks():
    v, col, f = (torch.from_numpy(a) for a in C.two_fans())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.mesh_components(f, 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.clean_mesh({"vertices": v, "colors": col, "faces": f})
    for bad in (f.long(), f[:, :2], f.reshape(-1), f.numpy()):
        with pytest.raises(ValueError, match="faces must be an int32"):
            mesh.mesh_components(bad, 9)
    with pytest.raises(ValueError):
        mesh.mesh_components(f, -1)
    for kw in (dict(min_faces=-1), dict(keep_largest=-1)):
        with pytest.raises(ValueError, match=">= 0"):
            mesh.clean_mesh({"vertices": v, "colors": col, "faces": f}, **kw)
    with pytest.raises(ValueError, match="vertices must be"):
        mesh.clean_mesh({"vertices": v.double(), "colors": col, "faces": f})
    with pytest.raises(ValueError, match="colors must be"):
        mesh.clean_mesh({"vertices": v, "colors": col[:5], "faces": f})
    with pytest.raises(ValueError, match=">= 0"):
        mesh.mesh_scan("nowhere", "nowhere", "nowhere.ply", 1.0, min_component=-2)
    assert mesh.MAX_ROUNDS == 64


def test_header_and_signatures():
    header = open(os.path.join(ROOT, "include", "cds_mvsnet_hip.h")).read()
    assert re.search(r"#define\s+CDS_MESH_CC_MAX_ROUNDS\s+64\b", header)
    for name, nargs in (("cds_mesh_cc_init", 3), ("cds_mesh_cc_hook", 6), ("cds_mesh_cc_jump", 3), ("cds_mesh_cc_count", 6),
                        ("cds_mesh_cc_mark", 8), ("cds_mesh_cc_gather", 15)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\);", header, re.M | re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name


def test_options_and_printed_line(capsys):
    ap = argparse.ArgumentParser()
    mesh.add_mesh_args(ap)
    args = ap.parse_args(["--mesh_voxel", "2"])
    assert (args.mesh_min_component, args.mesh_keep_largest) == (0, 0)
    args = ap.parse_args(["--mesh_voxel", "2", "--mesh_min_component", "50", "--mesh_keep_largest", "3"])
    assert (args.mesh_min_component, args.mesh_keep_largest) == (50, 3)
    base = ["--testpath", "x", "--testlist", "x", "--outdir", "x"]
    assert infer.parse_args(base + ["--fuse", "--mesh_voxel", "2", "--mesh_min_component", "9"]).mesh_min_component == 9
    assert infer.parse_args(base + ["--fuse", "--mesh_voxel", "2"]).mesh_keep_largest == 0
    for extra in (["--mesh_min_component", "9"], ["--mesh_keep_largest", "1"],                     # no mesh to clean
                  ["--mesh_voxel", "2", "--mesh_min_component", "-1"], ["--mesh_voxel", "2", "--mesh_keep_largest", "-1"]):
        with pytest.raises(SystemExit):
            infer.parse_args(base + ["--fuse"] + extra)
    for argv in (["--outdir", "x", "--testlist", "x"],                                            # neither mode
                 ["--outdir", "x", "--testlist", "x", "--mesh_voxel", "2", "--from_mesh", "y"],   # both
                 ["--outdir", "x", "--testlist", "x", "--mesh_voxel", "2"],                       # fusion needs the scenes
                 ["--outdir", "x", "--testlist", "x", "--from_mesh", "y", "--mesh_min_component", "-1"]):
        with pytest.raises(SystemExit):
            mesh.main(argv)
    capsys.readouterr()
    old = {"vertices": 7, "faces": 5, "blocks": 3}
    assert mesh.format_mesh(old) == "7 vertices, 5 faces, 3 blocks"                                # the line of a run without clean-up
    new = dict(old, clean={"components": (4, 1), "vertices": (20, 7), "faces": (30, 5), "largest": 5, "rounds": 2})
    line = mesh.format_mesh(new)
    assert line.startswith("7 vertices, 5 faces, 3 blocks") and "removed 3 of 4 components and 25 of 30 faces" in line
