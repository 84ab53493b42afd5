"""The kernels of csrc/mesh_fill.hip against the numpy restatement of their rule (mesh_fill_ref.py): vertices bit for
bit, colours, faces and the info exactly, and mesh_borders' outputs.  Then a property that needs no restatement (a punched sphere
is closed again and its caps face outwards) and the way to a filled mesh file through mesh_scan, the command line, --from_mesh and
infer --fuse --mesh_voxel --render_mesh."""
import filecmp
import functools
import os

import numpy as np
import pytest
import torch

import mesh_fill_ref as R
import mesh_ref as M
from cds_mvsnet_amd import _lib, fusion, infer, mesh, mvs_io, render
from test_mesh_gpu import VOXEL, _check_file, _child, _write_outputs
from test_mvs_io import _write_scene
from test_render_gpu import FUSE, _tree

pytestmark = pytest.mark.gpu

WINDOWS = [2 ** k + d for k in range(2, 7) for d in (-1, 0, 1)]         # 3, 4, 5, 7, 8, 9, ..., 63, 64, 65
NUMBERINGS = {"first": (0, False), "middle": (3, False), "last": (6, False), "against": (2, True)}

CASES = {"tetrahedron": R.open_tetrahedron, "cube": R.cube, "triangle": R.lone_triangle, "closed cube": lambda: R.cube(False),
         "ring": R.ring_strip, "ring with a hole": lambda: R.ring_strip(hole=5), "bow tie": R.bow_tie, "fin": R.fin,
         "flipped": R.flipped, "degenerate": R.with_degenerate_faces, "bits": R.odd_bits, "random": R.random_faces,
         "punched": lambda: R.random_punched_grid(3)}
CASES.update({f"hole {n}": functools.partial(R.grid_with_hole, n) for n in sorted(set(WINDOWS + [3, 4, 5, 8, 63, 64, 65]))})
CASES.update({f"patches {n}": functools.partial(R.patches, n) for n in (1, 255, 256, 257, 1000)})
CASES.update({f"leader {name}": functools.partial(lambda p, d: R.renumbered_loop(R.grid_with_hole(7), 7, p, d), *how)
              for name, how in NUMBERINGS.items()})


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}, expected {want.dtype} {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what} differs"


def _upload(v, c, f):
    return {"vertices": torch.from_numpy(np.ascontiguousarray(v)).cuda(), "colors": torch.from_numpy(np.ascontiguousarray(c)).cuda(),
            "faces": torch.from_numpy(np.ascontiguousarray(f)).cuda()}


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """A named mesh; built once, not to be modified."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _want(name, max_edges):
    return R.fill(*_mesh(name), max_edges)


@functools.lru_cache(maxsize=None)
def _want_borders(name):
    v, c, f = _mesh(name)
    return R.borders(f, len(v))


def _compare(got, info, wout, winfo, what):
    for k in ("vertices", "colors", "faces"):
        assert got[k].is_cuda and got[k].is_contiguous()
        _same(got[k].cpu().numpy(), wout[k], f"{what}: {k}")
    assert info == winfo, f"{what}: {info}, expected {winfo}"


def _run(name, max_edges):
    """fill_holes and mesh_borders of a named mesh against the restatement -> (the mesh made, its info)."""
    v, c, f = _mesh(name)
    what = f"{name}, max_edges {max_edges}"
    m = _upload(v, c, f)
    before = {k: t.clone() for k, t in m.items()}
    got, info = mesh.fill_holes(m, max_edges)
    assert all(torch.equal(m[k].view(torch.uint8), before[k].view(torch.uint8)) for k in m), f"{what}: the input changed"
    _compare(got, info, *_want(name, max_edges), what)
    if info["loops"] == 0:
        assert all(got[k] is m[k] for k in m), f"{what}: nothing filled, and not the input's own tensors"
    b, wb = mesh.mesh_borders(m["faces"], len(v)), _want_borders(name)
    _same(b["next"].cpu().numpy(), wb["next"], f"{what}: next")
    _same(b["regular"].cpu().numpy(), wb["regular"], f"{what}: regular")
    assert b["border_edges"] == wb["border_edges"] == info["border_edges"][0]
    return got, info


# ---------------------------------------------------------------------------------------------------------------- the cases
def test_solids_and_the_lone_triangle():
    got, info = _run("tetrahedron", 3)
    assert got["faces"][3].tolist() == [1, 2, 3] and info["border_edges"] == (3, 0) and info["vertices"] == (4, 4)
    got, info = _run("cube", 4)
    assert got["vertices"][8].tolist() == [1.0, 0.5, 0.5] and info["faces"] == (10, 14) and info["border_edges"] == (4, 0)
    assert R.signed_volume(got["vertices"].cpu().numpy(), got["faces"].cpu().numpy()) == 1.0
    assert mesh.mesh_borders(got["faces"], 9)["border_edges"] == 0
    assert _run("cube", 3)[1]["loops"] == 0
    got, info = _run("triangle", 3)
    assert got["faces"].tolist() == [[0, 1, 2], [0, 2, 1]] and mesh.mesh_borders(got["faces"], 3)["border_edges"] == 0


@pytest.mark.parametrize("n", [3, 4, 5, 8, 63, 64, 65])
def test_the_cap(n):
    """A hole of n edges in the 12 x 12 grid, whose own rim has 48: 64 is filled at max_edges 64 and 65 is not; the rim is filled
    at 64 and not at 47."""
    got, info = _run(f"hole {n}", 64)
    assert info["loops"] == (2 if n <= 64 else 1) and info["largest"] == (max(n, 48) if n <= 64 else 48)
    assert info["border_edges"] == (48 + n, 0 if n <= 64 else n)
    got, info = _run(f"hole {n}", 47)
    assert info["loops"] == (1 if n <= 47 else 0) and info["border_edges"][1] == 48 + (0 if n <= 47 else n)
    if n == 5:
        assert _run("hole 5", 3)[1]["loops"] == 0 and _run("hole 5", 4)[1]["loops"] == 0
        assert _run("hole 5", 4096)[1]["loops"] == 2
    if n == 3:
        assert _run("hole 3", 3)[1]["loops"] == 1 and _run("hole 4", 4)[1]["loops"] == 1


@pytest.mark.parametrize("n", WINDOWS)
def test_doubling_windows(n):
    """Loops of 2^k - 1, 2^k and 2^k + 1 edges at max_edges equal to the length and one less: on either side of a round of the
    doubling, the loop is found when it fits and left when it does not."""
    assert _run(f"hole {n}", n)[1]["loops"] == 1 + (n >= 48)                # the grid's own rim of 48 edges is a loop too
    if n > 3:
        assert _run(f"hole {n}", n - 1)[1]["loops"] == (n - 1 >= 48)


@pytest.mark.parametrize("name", list(NUMBERINGS))
def test_leader_rule(name):
    """One mesh with a 7-edge hole under four numberings: the smallest vertex first, in the middle and last on the loop, and one
    in which next runs against ascending indices."""
    v, c, f = _mesh(f"leader {name}")
    path = R.loop_of(f, len(v), 7)
    if name == "against":
        assert path[1:] == sorted(path[1:], reverse=True)
    else:
        assert path == sorted(path)
    got, info = _run(f"leader {name}", 8)
    assert info["loops"] == 1 and got["faces"][-7].tolist() == [path[1], path[0], len(v)]


def test_pruning_on_long_rims():
    """A ring-shaped strip whose two rims have 10 000 edges each: nothing is filled at max_edges 64; with one hole of 5 edges
    punched into it exactly that one is.  A prune that loses a loop fails here."""
    got, info = _run("ring", 64)
    assert info["loops"] == 0 and info["border_edges"] == (20000, 20000)
    got, info = _run("ring with a hole", 64)
    assert info["loops"] == 1 and info["largest"] == 5 and info["border_edges"] == (20005, 20000) and info["faces"][1] == info["faces"][0] + 5


@pytest.mark.parametrize("count", [1, 255, 256, 257, 1000])
def test_launch_shapes(count):
    """Separate 4-edge holes, each in its own patch, interleaved in memory: the new vertices and faces come in ascending label
    order."""
    got, info = _run(f"patches {count}", 4)
    v, c, f = _mesh(f"patches {count}")
    assert info["loops"] == count and info["vertices"] == (len(v), len(v) + count) and info["faces"] == (len(f), len(f) + 4 * count)
    new = got["faces"][len(f):].cpu().numpy().reshape(count, 4, 3)
    assert (new[:, :, 2] == (len(v) + np.arange(count))[:, None]).all()
    labels = new[:, :, 1].min(1)
    assert (new[:, 0, 1] == labels).all() and (np.diff(labels) > 0).all()
    assert _run(f"patches {count}", 12)[1]["loops"] == 2 * count


def test_what_must_stay_open(monkeypatch):
    got, info = _run("bow tie", 23)
    assert info["loops"] == 0 and info["border_edges"] == (32, 32)
    assert not mesh.mesh_borders(got["faces"], 49)["regular"][3 * 7 + 3]
    got, info = _run("fin", 23)                                          # an edge held by three faces; the hole elsewhere is filled
    assert info["loops"] == 1 and info["border_edges"] == (30, 26)
    got, info = _run("flipped", 23)                                      # two faces hold an edge in the same direction
    assert info["loops"] == 1 and info["border_edges"] == (28, 24)
    got, info = _run("degenerate", 8)                                    # (a, a, b): copied through and otherwise ignored
    assert info["loops"] == 1 and info["largest"] == 5
    _run("random", 16)
    _run("punched", 16)
    # a face with an index outside the vertices reaches the entry points when the wrapper's range check is taken away
    v, c, f = _mesh("degenerate")
    bad = np.insert(f, [0, 31, len(f)], np.array([[0, 1, len(v)], [-1, 0, 4], [3, 2 ** 31 - 1, 5]], np.int32), axis=0)
    monkeypatch.setattr(mesh, "_check_index_range", lambda *a: None)
    got, info = mesh.fill_holes(_upload(v, c, bad), 8)
    _compare(got, info, *R.fill(v, c, bad, 8), "faces outside the vertices")
    assert info["loops"] == 1 and torch.equal(got["faces"][:len(bad)].cpu(), torch.from_numpy(bad))
    b, wb = mesh.mesh_borders(torch.from_numpy(bad).cuda(), len(v)), _want_borders("degenerate")
    _same(b["next"].cpu().numpy(), wb["next"], "next")
    assert b["border_edges"] == wb["border_edges"]


def test_bits():
    """-0.0, denormals, an infinity and a NaN on a rim: the input rows keep their bits, the new vertices have the restatement's;
    colour means that fall on .5 round up."""
    v, c, f = _mesh("bits")
    assert np.isnan(v).any() and np.isinf(v).any() and np.signbit(v[v == 0]).any() and (np.abs(v[v != 0]) < 1e-38).any()
    got, info = _run("bits", 16)
    assert info["loops"] == 2 and info["vertices"] == (169, 171)
    _same(got["vertices"][:169].cpu().numpy(), v, "input rows")
    new = got["vertices"][169:].cpu().numpy()
    assert np.isinf(new[0, 0]) and new[0:1, 1].view(np.uint32)[0] == 0x7fc00000 and new[0, 2] == 0.25
    assert got["colors"][169:].tolist() == [[1, 201, 255], [2, 3, 3]]


def test_degenerate_inputs_and_errors():
    f0 = np.zeros((0, 3), np.int32)
    v5, c5 = np.arange(15, dtype=np.float32).reshape(5, 3), np.arange(15, dtype=np.uint8).reshape(5, 3)
    for v, c, f in ((v5[:0], c5[:0], f0), (v5, c5, f0), R.cube(False)):
        m = _upload(v, c, f)
        got, info = mesh.fill_holes(m, 16)
        assert all(got[k] is m[k] for k in m)
        assert info == R.fill(v, c, f, 16)[1] and info["loops"] == 0 and info["border_edges"] == (0, 0)
        b = mesh.mesh_borders(m["faces"], len(v))
        assert b["border_edges"] == 0 and not b["regular"].any() and (b["next"] == -1).all() and b["next"].dtype == torch.int32
    for name in ("random", "patches 257"):                               # two runs give equal bytes
        m = _upload(*_mesh(name))
        (a, ia), (b, ib) = mesh.fill_holes(m, 12), mesh.fill_holes(m, 12)
        assert ia == ib and all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)
    m = _upload(*_mesh("cube"))
    for k in ("vertices", "colors", "faces"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mesh.fill_holes(dict(m, **{k: m[k].cpu()}), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.mesh_borders(m["faces"].cpu(), 8)
    for bad in (dict(m, vertices=m["vertices"].double()), dict(m, colors=m["colors"].int()), dict(m, faces=m["faces"].long()),
                dict(m, faces=m["faces"].reshape(-1))):
        with pytest.raises(ValueError, match="must be"):
            mesh.fill_holes(bad, 4)
    with pytest.raises(ValueError, match="must be an int32"):
        mesh.mesh_borders(m["faces"].long(), 8)
    with pytest.raises(ValueError, match="outside the 7 vertices"):
        mesh.mesh_borders(m["faces"], 7)
    for bad in (2, 4097, 3.5, True):
        with pytest.raises(ValueError, match="max_edges must be an int in 3..4096"):
            mesh.fill_holes(m, bad)


def test_entry_points_refuse_what_the_wrapper_never_sends():
    lib = _lib.load()
    assert lib.cds_mesh_fill_max_edges() == mesh.MAX_FILL_EDGES
    p = torch.zeros(64, dtype=torch.int64, device="cuda").data_ptr()
    q = p + 256
    E = _lib.EINVAL
    keys, bor, init, dbl = lib.cds_mesh_fill_keys, lib.cds_mesh_fill_borders, lib.cds_mesh_fill_init, lib.cds_mesh_fill_double
    walk, emit = lib.cds_mesh_fill_walk, lib.cds_mesh_fill_emit
    assert keys(None, 1, 8, p, None) == E and keys(p, 1, 8, None, None) == E and keys(p, -1, 8, p, None) == E
    assert keys(p, 1, -1, p, None) == E and keys(p, 1, 2 ** 31, p, None) == E and keys(p, 2 ** 31 // 3 + 1, 8, p, None) == E
    assert keys(None, 0, 8, None, None) == 0
    assert bor(None, 3, 8, p, p, p, p, None) == E and bor(p, 3, 8, None, p, p, p, None) == E and bor(p, 3, 8, p, None, p, p, None) == E
    assert bor(p, 3, 8, p, p, None, p, None) == E and bor(p, 3, 8, p, p, p, None, None) == E and bor(p, -1, 8, p, p, p, p, None) == E
    assert bor(p, 3, -1, p, p, p, p, None) == E and bor(p, 2 ** 31, 8, p, p, p, p, None) == E
    assert bor(None, 0, 8, None, None, None, None, None) == 0
    good = [p, p, p, p, p, p, p, q, q]
    for k in range(9):
        assert init(2, *[None if i == k else x for i, x in enumerate(good)], None) == E
    assert init(2, p, p, p, p, p, p, p, p, p, None) == E                 # the same arrays on both sides
    assert init(-1, *good, None) == E and init(2 ** 31, *good, None) == E and init(0, *[None] * 9, None) == 0
    good = [p, 2, 8, p, p, q, q]
    for k in (0, 3, 4, 5, 6):
        assert dbl(*[None if i == k else x for i, x in enumerate(good)], None) == E
    assert dbl(p, 2, 8, p, p, p, p, None) == E and dbl(p, 9, 8, p, p, q, q, None) == E and dbl(p, -1, 8, p, p, q, q, None) == E
    assert dbl(p, 2, 2 ** 31, p, p, q, q, None) == E and dbl(None, 0, 8, None, None, None, None, None) == 0
    good = [p, p, 8, p, p, p, p, 2, 16, p, p, p]
    for k in (0, 1, 3, 4, 5, 6, 9, 10, 11):
        assert walk(*[None if i == k else x for i, x in enumerate(good)], None) == E
    for k, bad in ((2, -1), (2, 2 ** 31), (7, -1), (7, 9), (8, 2), (8, 4097)):
        assert walk(*[bad if i == k else x for i, x in enumerate(good)], None) == E
    assert walk(None, None, 8, None, None, None, None, 0, 16, None, None, None, None) == 0
    good = [p, p, 8, 4, p, 2, 16, p, p, p, p, p, 1, 4, p, p, p]
    for k in (0, 1, 4, 7, 8, 9, 10, 11, 13 + 1, 13 + 2, 13 + 3):
        assert emit(*[None if i == k else x for i, x in enumerate(good)], None) == E, k
    for k, bad in ((2, -1), (3, -1), (5, -1), (5, 9), (6, 2), (6, 4097), (12, -1), (13, -1), (12, 2 ** 31), (13, 2 ** 31 - 2)):
        assert emit(*[bad if i == k else x for i, x in enumerate(good)], None) == E, k
    assert emit(None, None, 8, 4, None, 0, 16, None, None, None, None, None, 0, 0, None, None, None, None) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- a property without a restatement
def _sphere_views():
    """The 26-camera sphere of mesh_ref.sphere_scene (48 x 48 maps) as the records that filter_depth(collect=...) gathers."""
    sc = M.sphere_case()[0]
    counts = [int((m != 0).sum()) for m in sc["masks"]]
    pts = np.split(sc["points"], np.cumsum(counts)[:-1])
    views = [{"depth": torch.from_numpy(sc["depths"][v]).cuda(), "mask": torch.from_numpy(sc["masks"][v] != 0).cuda(),
              "image": torch.from_numpy(sc["images"][v]).cuda(), "cam": torch.from_numpy(sc["cams"][v]),
              "points": torch.from_numpy(pts[v]).cuda()} for v in range(len(counts))]
    return sc, views


def test_a_punched_sphere_is_closed_again_and_its_caps_face_outwards():
    sc, views = _sphere_views()
    s = sc["voxel"]
    m, vol = mesh.mesh_views(views, s, 2.5 * s, 2)
    v, c, f = (m[k].cpu().numpy() for k in ("vertices", "colors", "faces"))
    assert not mesh.mesh_adjacency(m["faces"], len(v))["boundary"].any() and M.topology(f, len(v))["euler"] == 2
    # 5 vertices far from each other: the rims of their holes share nothing
    direction = (v - sc["centre"]) / np.linalg.norm(v - sc["centre"], axis=1, keepdims=True)
    poles = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [-0.6, -0.8, 0]], np.float64)
    chosen = [int(np.argmax(direction @ p)) for p in poles]
    gone = np.isin(f, chosen).any(1)
    rims = [int(np.isin(f, x).any(1).sum()) for x in chosen]
    assert len(set(chosen)) == 5 and gone.sum() == sum(rims) and 3 <= min(rims) and max(rims) <= 16
    punched = dict(m, faces=torch.from_numpy(f[~gone]).cuda())
    assert mesh.mesh_borders(punched["faces"], len(v))["border_edges"] == sum(rims)
    got, info = mesh.fill_holes(punched, 16)
    assert info["loops"] == 5 and info["border_edges"] == (sum(rims), 0) and info["largest"] == max(rims)
    assert not mesh.mesh_adjacency(got["faces"], got["vertices"].shape[0])["boundary"].any()
    gv, gf = got["vertices"].cpu().numpy().astype(np.float64), got["faces"].cpu().numpy()
    assert M.topology(gf, len(gv))["euler"] == 2 + 5 - 5                  # five vertices left unused, five caps added
    new = gv[gf[len(f) - gone.sum():]]
    normal = np.cross(new[:, 1] - new[:, 0], new[:, 2] - new[:, 0])
    radius = new.mean(1) - sc["centre"]
    assert len(new) == sum(x if x > 3 else 1 for x in rims) and ((normal * radius).sum(1) > 0).all()
    _compare(got, info, *R.fill(v, c, f[~gone], 16), "punched sphere")


# -------------------------------------------------------------------------------------------------------------- end to end
def _no_fill(*a, **k):
    raise AssertionError("fill_holes ran without --mesh_fill_holes")


def _write(path, m):
    mesh.write_mesh_ply(path, *(m[k].cpu().numpy() for k in ("vertices", "colors", "faces")))


def test_mesh_scan_and_command_line(tmp_path, capsys, monkeypatch):
    """The synthetic scan of test_mesh_gpu (3 views of 24 x 40): mesh_scan(fill_holes=N) writes fill_holes of the mesh it writes
    without; clean, fill, smooth, simplify through mesh_scan are the four library calls in that order; mesh.main with --mesh_voxel
    and with --from_mesh write the same file; without the option nothing of this runs and no byte changes."""
    scan, pairs = _write_outputs(tmp_path)
    out = tmp_path / "out"
    kw = dict(thres_view=1)
    lst = str(tmp_path / "list.txt")
    cli = ["--testpath", str(tmp_path / "in"), "--outdir", str(out), "--testlist", lst, "--thres_view", "1", "--mesh_voxel", str(VOXEL)]
    views: list = []
    fusion.filter_depth(str(pairs), str(scan), None, collect=views, **kw)
    untouched = str(tmp_path / "untouched_mesh.ply")
    _write(untouched, mesh.mesh_views(views, VOXEL)[0])
    plain = str(tmp_path / "plain_mesh.ply")
    with monkeypatch.context() as mp:
        mp.setattr(mesh, "fill_holes", _no_fill)
        info0 = mesh.mesh_scan(str(pairs), str(scan), plain, VOXEL, **kw)
        zero = mesh.mesh_scan(str(pairs), str(scan), str(tmp_path / "zero_mesh.ply"), VOXEL, fill_holes=0, **kw)
        mesh.main(cli)
        assert filecmp.cmp(str(out / "scan1_mesh.ply"), untouched, shallow=False)
    assert filecmp.cmp(plain, untouched, shallow=False) and filecmp.cmp(str(tmp_path / "zero_mesh.ply"), untouched, shallow=False)
    assert sorted(info0) == sorted(zero) == ["blocks", "cloud", "faces", "mesh", "vertices"]
    saved = str(tmp_path / "saved_mesh.ply")
    os.replace(out / "scan1_mesh.ply", saved)
    arrays = mesh.read_mesh_ply(plain)
    wout, winfo = R.fill(*arrays, 16)
    print(f"the scan's mesh: {winfo}")
    assert winfo["loops"] > 0 and winfo["border_edges"][1] > 0           # holes are filled and the scan's own rim is not
    # mesh_scan(fill_holes=16) against fill_holes of the loaded file, and against the restatement
    filled, finfo = mesh.fill_holes(mesh.load_mesh(plain), 16)
    lib_ply = str(tmp_path / "lib_mesh.ply")
    _write(lib_ply, filled)
    direct = str(tmp_path / "direct_mesh.ply")
    info = mesh.mesh_scan(str(pairs), str(scan), direct, VOXEL, fill_holes=16, **kw)
    assert filecmp.cmp(direct, lib_ply, shallow=False) and not filecmp.cmp(direct, plain, shallow=False)
    assert info["fill"] == finfo == winfo and info["blocks"] == info0["blocks"] and "clean" not in info
    v, c, f = _check_file(direct)
    for got, k in ((v, "vertices"), (c, "colors"), (f, "faces")):
        _same(got, wout[k], f"mesh_scan: {k}")
    assert np.array_equal(info["mesh"]["faces"].cpu().numpy(), f)                                   # what render_scan gets
    # clean -> fill -> smooth -> simplify
    cell = 2.0 * VOXEL
    a, ia = mesh.clean_mesh(info0["mesh"], 5, 0)
    b, ib = mesh.fill_holes(a, 16)
    d, id_ = mesh.smooth_mesh(b, 3)
    e, ie = mesh.simplify_mesh(d, cell, "quadric")
    chain = str(tmp_path / "chain_mesh.ply")
    _write(chain, e)
    four = str(tmp_path / "four_mesh.ply")
    info = mesh.mesh_scan(str(pairs), str(scan), four, VOXEL, min_component=5, simplify=cell, smooth=3, fill_holes=16, **kw)
    assert filecmp.cmp(four, chain, shallow=False)
    assert info["fill"] == ib and info["smooth"] == dict(id_, limit=0.0) and info["simplify"] == ie and ib["loops"] > 0
    assert id_["vertices"] == ib["vertices"][1]                                                      # the smoothing saw the caps
    # the command line: --mesh_voxel in this process and in a child, --from_mesh on the saved mesh
    capsys.readouterr()
    res = mesh.main(cli + ["--mesh_fill_holes", "16"])
    line = capsys.readouterr().out
    assert res["scan1"]["fill"] == winfo and filecmp.cmp(str(out / "scan1_mesh.ply"), direct, shallow=False)
    assert (f"filled {winfo['loops']} holes of at most 16 edges (the largest has {winfo['largest']}), border edges "
            f"{winfo['border_edges'][0]} -> {winfo['border_edges'][1]}") in line
    os.remove(out / "scan1_mesh.ply")
    stdout = _child("cds_mvsnet_amd.mesh", cli + ["--mesh_fill_holes", "16"])
    assert filecmp.cmp(str(out / "scan1_mesh.ply"), direct, shallow=False) and f"filled {winfo['loops']} holes" in stdout
    os.remove(out / "scan1_mesh.ply")
    res = mesh.main(["--from_mesh", saved, "--outdir", str(out), "--testlist", lst, "--mesh_fill_holes", "16"])
    assert filecmp.cmp(str(out / "scan1_mesh.ply"), direct, shallow=False)
    assert res["scan1"]["fill"] == winfo and "clean" not in res["scan1"]
    res = mesh.main(["--from_mesh", saved, "--outdir", str(out), "--testlist", lst, "--mesh_fill_holes", "16", "--mesh_smooth", "3",
                     "--mesh_min_component", "5", "--mesh_simplify", str(cell)])
    assert filecmp.cmp(str(out / "scan1_mesh.ply"), chain, shallow=False) and res["scan1"]["fill"] == ib
    assert filecmp.cmp(saved, untouched, shallow=False)                                             # the source is not touched
    with pytest.raises(SystemExit):
        mesh.main(["--outdir", str(out), "--testlist", lst, "--mesh_fill_holes", "16"])


def test_infer_fill_and_render(tmp_path, capsys):
    """infer --fuse --mesh_voxel --mesh_fill_holes 16 --render_mesh on a scene of test_mvs_io._write_scene (3 views of 128 x 160, an
    untrained network, the loose settings of test_mesh_gpu.test_infer_fuse_mesh): the mesh file is the restatement's fill of the
    file of the run without the option (in which fill_holes is not called), every other file is that run's, and depth_mesh is
    render_scan of the filled file."""
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
        mp.setattr(mesh, "fill_holes", _no_fill)
        infer.main(base + ["--outdir", plain])
    arrays = mesh.read_mesh_ply(os.path.join(plain, "scanA_mesh.ply"))
    wout, winfo = R.fill(*arrays, 16)
    print(f"the scene's mesh: {winfo}")
    assert winfo["loops"] > 0
    out = str(tmp_path / "filled")
    capsys.readouterr()
    infer.main(base + ["--outdir", out, "--mesh_fill_holes", "16", "--render_mesh"])
    lines = capsys.readouterr().out.splitlines()
    v, c, f = _check_file(os.path.join(out, "scanA_mesh.ply"))
    for got, k in ((v, "vertices"), (c, "colors"), (f, "faces")):
        _same(got, wout[k], f"infer: {k}")
    line = [ln for ln in lines if "scanA_mesh.ply" in ln]
    assert line and f"filled {winfo['loops']} holes of at most 16 edges" in line[0]
    for name in _tree(plain):
        if name != "scanA_mesh.ply":
            assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    scan = os.path.join(out, "scanA")
    render.render_scan(scan, os.path.join(out, "scanA_mesh.ply"), os.path.join(root, "scanA"), subdir="again")
    render.render_scan(scan, os.path.join(plain, "scanA_mesh.ply"), os.path.join(root, "scanA"), subdir="open")
    differ = 0
    for i in range(3):
        a = mvs_io.read_pfm(os.path.join(scan, "depth_mesh", f"{i:08d}.pfm"))[0]
        b = mvs_io.read_pfm(os.path.join(scan, "again", f"{i:08d}.pfm"))[0]
        d = mvs_io.read_pfm(os.path.join(scan, "open", f"{i:08d}.pfm"))[0]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (a > 0).any()
        differ += int((a.view(np.uint32) != d.view(np.uint32)).sum())
    print(f"{winfo['loops']} holes filled; {differ} pixels of depth_mesh change")
