"""The component kernels of csrc/mesh_clean.hip against the numpy restatement of their rule (mesh_clean_ref.py),
exactly: labels, component lists, counts and the cleaned mesh are integers or copied bits.  Then the way to a cleaned mesh file
through mesh_scan, the command line and infer --fuse --mesh_voxel."""
import filecmp
import os

import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_ref as M
from cds_mvsnet_amd import _lib, infer, mesh, mvs_io, render
from test_mesh_gpu import VOXEL, _check_file, _child, _write_outputs
from test_mvs_io import _write_scene
from test_render_gpu import FUSE, _tree

pytestmark = pytest.mark.gpu


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}, expected {want.dtype} {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what} differs"


def _components(faces, nv, what):
    """mesh_components on the device against the restatement -> the round count."""
    got = mesh.mesh_components(torch.from_numpy(np.ascontiguousarray(faces)).cuda(), nv)
    want = C.components(faces, nv)
    for k in ("label", "components", "faces"):
        assert got[k].is_cuda
        _same(got[k].cpu().numpy(), want[k], f"{what}: {k}")
    rounds = got["rounds"]
    print(f"{what}: {len(faces)} faces, {nv} vertices, {len(want['components'])} components, {rounds} rounds")
    assert isinstance(rounds, int) and (1 <= rounds <= mesh.MAX_ROUNDS if len(faces) and nv else rounds == 0)
    return rounds


def _upload(v, c, f):
    return {"vertices": torch.from_numpy(v).cuda(), "colors": torch.from_numpy(c).cuda(), "faces": torch.from_numpy(f).cuda()}


def _clean(v, c, f, what, **kw):
    """clean_mesh on the device against the restatement: the three arrays and the info -> (mesh as numpy, info)."""
    got, info = mesh.clean_mesh(_upload(v, c, f), **kw)
    want, winfo = C.clean(v, c, f, **kw)
    out = {}
    for k in ("vertices", "colors", "faces"):
        assert got[k].is_cuda and got[k].is_contiguous()
        out[k] = got[k].cpu().numpy()
        _same(out[k], want[k], f"{what} {kw}: {k}")
    rounds = info.pop("rounds")
    assert info == winfo, f"{what} {kw}: {info}, expected {winfo}"
    assert 0 <= rounds <= mesh.MAX_ROUNDS
    return out, info


# ----------------------------------------------------------------------------------------------------------- launch shapes
@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_isolated_triangles(n_faces):
    v, c, f = C.isolated_triangles(n_faces, seed=n_faces)
    _components(f, len(v), f"{n_faces} triangles")
    _clean(v, c, f, "triangles")
    _clean(v, c, f, "triangles", min_faces=2)                            # every component has one face: nothing stays
    _clean(v, c, f, "triangles", keep_largest=max(1, n_faces // 3))      # all counts tie: the lowest labels stay


def test_many_more_vertices_than_referenced():
    v, c, f = C.isolated_triangles(70, n_vertices=100003, seed=7)
    assert len(np.unique(f)) == 210
    _components(f, len(v), "sparse")
    out, info = _clean(v, c, f, "sparse")
    assert info["vertices"] == (100003, 210) and info["components"] == (100003 - 140, 70)


def test_empty_meshes_make_no_launch(monkeypatch):
    def no_launch():
        raise AssertionError("the library was loaded: a launch was about to happen")
    monkeypatch.setattr(mesh._lib, "load", no_launch)
    f0 = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    for nv in (0, 5):
        got = mesh.mesh_components(f0, nv)
        want = C.components(np.zeros((0, 3), np.int32), nv)
        for k in ("label", "components", "faces"):
            _same(got[k].cpu().numpy(), want[k], f"F = 0, V = {nv}: {k}")
        assert got["rounds"] == 0
        v, c = np.zeros((nv, 3), np.float32), np.zeros((nv, 3), np.uint8)
        out, info = _clean(v, c, np.zeros((0, 3), np.int32), f"F = 0, V = {nv}")
        assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3) and info["vertices"] == (nv, 0)


# ------------------------------------------------------------------------------------------------------------ the CPU cases
def test_sphere_and_debris():
    sphere = M.analytic_case("sphere")[1]
    _components(sphere["faces"], len(sphere["vertices"]), "sphere")
    v, c, f = C.sphere_with_debris()
    _components(f, len(v), "sphere and two tetrahedra")
    out, info = _clean(v, c, f, "debris", min_faces=5)
    for k in ("vertices", "colors", "faces"):
        _same(out[k], sphere[k], f"the sphere back: {k}")
    assert info["largest"] == 4568 and info["components"] == (3, 1)
    out, _ = _clean(v, c, f, "debris", keep_largest=2)
    _same(out["faces"], f[:4572], "the sphere and the first tetrahedron")
    _clean(v, c, f, "debris", min_faces=4, keep_largest=1)
    _clean(v, c, f, "debris", min_faces=5, keep_largest=3)
    for mf in (0, 1):                                                    # identity
        out, _ = _clean(v, c, f, "debris", min_faces=mf)
        for k, a in (("vertices", v), ("colors", c), ("faces", f)):
            _same(out[k], a, f"identity: {k}")


def test_fans_degenerate_duplicate_unreferenced():
    v, c, f = C.two_fans()
    _components(f, len(v), "two fans")
    assert mesh.mesh_components(torch.from_numpy(f).cuda(), 9)["components"].tolist() == [0]
    _clean(v, c, f, "two fans", min_faces=6)
    _clean(v, c, f, "two fans", min_faces=7)
    v, c, f = C.odd_faces()
    _components(f, len(v), "odd faces")
    for kw in (dict(), dict(min_faces=3), dict(keep_largest=1), dict(keep_largest=3), dict(min_faces=2, keep_largest=2)):
        _clean(v, c, f, "odd faces", **kw)


# ------------------------------------------------------------------------------------------------------------ convergence
@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
def test_strip_of_65536_vertices(order):
    """One component of 2^16 vertices whose graph distance is 2^15: label propagation alone would need that many rounds along
    the ascending numbering; hooking roots and pointer jumping settle it in a few."""
    f = C.strip(1 << 16, order, seed=11)
    rounds = _components(f, 1 << 16, f"strip, {order}")
    assert rounds <= mesh.MAX_ROUNDS


def test_one_dominant_component_among_many():
    f, nv = C.strip_and_triangles(1 << 16, 10000)
    _components(f, nv, "strip and 10000 triangles")
    rng = np.random.default_rng(3)
    v, c = rng.normal(size=(nv, 3)).astype(np.float32), rng.integers(0, 256, (nv, 3)).astype(np.uint8)
    out, info = _clean(v, c, f, "strip and triangles", min_faces=2)
    assert info["faces"] == (len(f), (1 << 16) - 2) and info["components"] == (10001, 1)
    _clean(v, c, f, "strip and triangles", keep_largest=5001)


@pytest.mark.parametrize("n_faces", [300, 1000, 3000])
def test_random_graphs(n_faces):
    f = C.random_faces(2000, n_faces, seed=n_faces)
    _components(f, 2000, f"random, F = {n_faces}")
    rng = np.random.default_rng(n_faces)
    v, c = rng.normal(size=(2000, 3)).astype(np.float32), rng.integers(0, 256, (2000, 3)).astype(np.uint8)
    _clean(v, c, f, "random", min_faces=3)
    _clean(v, c, f, "random", min_faces=2, keep_largest=4)


# -------------------------------------------------------------------------------------------------------------- selection
def test_selection_ties_empty_result_and_both_options(tmp_path):
    # components of 2, 3, 3, 1, 3 faces at labels 0, 4, 9, 14, 17: fans around the first vertex of each
    sizes, faces, at = [2, 3, 3, 1, 3], [], 0
    for n in sizes:
        faces += [[at, at + k + 1, at + k + 2] for k in range(n)]
        at += n + 2
    f = np.array(faces, np.int32)
    rng = np.random.default_rng(9)
    v, c = rng.normal(size=(at, 3)).astype(np.float32), rng.integers(0, 256, (at, 3)).astype(np.uint8)
    got = mesh.mesh_components(torch.from_numpy(f).cuda(), at)
    assert got["components"].tolist() == [0, 4, 9, 14, 17] and got["faces"].tolist() == sizes
    out, info = _clean(v, c, f, "ties", keep_largest=2)                  # three components tie at 3 faces: labels 4 and 9 win
    _same(out["vertices"], v[4:14], "ties: the vertices of labels 4 and 9")
    _same(out["faces"], f[2:8] - 4, "ties: their faces")
    out, info = _clean(v, c, f, "ties", keep_largest=4)
    assert info["faces"] == (12, 11) and info["components"] == (5, 4)
    out, info = _clean(v, c, f, "both", min_faces=3, keep_largest=4)     # the 2-face component is among the 4 but too small
    assert info["faces"] == (12, 9)
    out, info = _clean(v, c, f, "both", min_faces=1, keep_largest=1)
    _same(out["faces"], f[2:5] - 4, "both: label 4 alone")
    out, info = _clean(v, c, f, "nothing", min_faces=4)                  # above every count
    assert info == {"components": (5, 0), "vertices": (at, 0), "faces": (12, 0), "largest": 3}
    path = str(tmp_path / "empty_mesh.ply")
    mesh.write_mesh_ply(path, out["vertices"], out["colors"], out["faces"])
    ve, ce, fe = _check_file(path)
    assert ve.shape == (0, 3) and fe.shape == (0, 3)


def test_order_and_bits():
    """Kept faces and vertices keep their relative order; positions come through as bits: -0.0, a denormal, NaNs with payloads,
    infinities."""
    f, nv = C.strip_and_triangles(1 << 8, 40)
    rng = np.random.default_rng(4)
    v = rng.normal(size=(nv, 3)).astype(np.float32)
    special = np.array([0x80000000, 0x00000001, 0x7fc00000, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000, 0x807fffff], np.uint32)
    v.reshape(-1)[:: 5][: 8 * 20] = np.tile(special, 20).view(np.float32)
    c = rng.integers(0, 256, (nv, 3)).astype(np.uint8)
    out, info = _clean(v, c, f, "bits")                                  # everything kept
    _same(out["vertices"], v, "bits: identity")
    out, info = _clean(v, c, f, "bits", keep_largest=1)                  # the strip: the first 256 vertices
    _same(out["vertices"], v[:256], "bits: the strip")
    assert np.isnan(out["vertices"]).any() and (np.diff(out["faces"][:, 0]) == 1).all()
    f2 = np.concatenate([f[f[:, 0] < 256][::-1][:100], f])               # strip faces again, backwards: sorted by nothing
    out, info = _clean(v, c, f2, "order", min_faces=2)
    kept = f2[f2[:, 0] < 256]                                            # the triangles have one face each and go
    _same(out["faces"], kept, "order: the strip's faces as they stood")


# ------------------------------------------------------------------------------------------------------------------ errors
def test_errors():
    v, c, f = C.two_fans()
    m = _upload(v, c, f)
    for bad in (np.array([[0, 1, 9]], np.int32), np.array([[0, -1, 2]], np.int32)):
        tf = torch.from_numpy(bad).cuda()
        with pytest.raises(ValueError, match="outside the 9 vertices"):
            mesh.mesh_components(tf, 9)
        with pytest.raises(ValueError, match="outside the 9 vertices"):
            mesh.clean_mesh(dict(m, faces=tf))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.mesh_components(m["faces"].cpu(), 9)
    for k in ("vertices", "colors", "faces"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mesh.clean_mesh(dict(m, **{k: m[k].cpu()}))
    for bad in (m["faces"].long(), m["faces"][:, :2], m["faces"].reshape(-1)):
        with pytest.raises(ValueError):
            mesh.mesh_components(bad, 9)
        with pytest.raises(ValueError):
            mesh.clean_mesh(dict(m, faces=bad))
    with pytest.raises(ValueError):
        mesh.clean_mesh(dict(m, vertices=m["vertices"].double()))
    with pytest.raises(ValueError):
        mesh.clean_mesh(dict(m, colors=m["colors"][:-1]))
    for kw in (dict(min_faces=-1), dict(keep_largest=-1)):
        with pytest.raises(ValueError, match=">= 0"):
            mesh.clean_mesh(m, **kw)


def test_entry_points_skip_what_the_wrapper_never_sends():
    """A face with an index outside the vertices is skipped by every kernel: the labels, counts and flags are those of the mesh
    without it.  Null pointers and sizes out of range are CDS_EINVAL."""
    lib = _lib.load()
    good = np.array([[0, 1, 2], [4, 5, 6], [2, 3, 3]], np.int32)
    bad = np.array([[0, 1, 2], [7, 8, 1], [4, 5, 6], [-1, 0, 4], [2, 3, 3], [0, 4, 2 ** 31 - 1]], np.int32)
    nv = 8
    res = {}
    for name, faces in (("good", good), ("bad", bad)):
        tf = torch.from_numpy(faces).cuda()
        nf = len(faces)
        parent = torch.empty(nv, dtype=torch.int32, device="cuda")
        count = torch.zeros(nv, dtype=torch.int32, device="cuda")
        changed = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert lib.cds_mesh_cc_init(parent.data_ptr(), nv, None) == 0
        assert lib.cds_mesh_cc_hook(tf.data_ptr(), nf, nv, parent.data_ptr(), changed.data_ptr(), None) == 0
        assert lib.cds_mesh_cc_jump(parent.data_ptr(), nv, None) == 0
        assert lib.cds_mesh_cc_count(tf.data_ptr(), nf, nv, parent.data_ptr(), count.data_ptr(), None) == 0
        keep = torch.ones(nv, dtype=torch.uint8, device="cuda")
        fk = torch.full((nf,), 7, dtype=torch.uint8, device="cuda")
        vk = torch.zeros(nv, dtype=torch.uint8, device="cuda")
        assert lib.cds_mesh_cc_mark(tf.data_ptr(), nf, nv, parent.data_ptr(), keep.data_ptr(), fk.data_ptr(), vk.data_ptr(), None) == 0
        torch.cuda.synchronize()
        res[name] = (parent.tolist(), count.tolist(), vk.tolist(), fk.tolist(), int(changed))
    assert res["good"][:3] == res["bad"][:3] == ([0, 0, 0, 0, 4, 4, 4, 7], [2, 0, 0, 0, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 0])
    assert res["good"][3] == [1, 1, 1] and res["bad"][3] == [1, 0, 1, 0, 1, 0] and res["good"][4] == res["bad"][4] == 1
    p = torch.zeros(8, dtype=torch.int32, device="cuda").data_ptr()
    E = _lib.EINVAL
    assert lib.cds_mesh_cc_init(None, 8, None) == E and lib.cds_mesh_cc_init(p, -1, None) == E
    assert lib.cds_mesh_cc_init(p, 2 ** 31, None) == E and lib.cds_mesh_cc_init(None, 0, None) == 0
    assert lib.cds_mesh_cc_hook(None, 1, 8, p, p, None) == E and lib.cds_mesh_cc_hook(p, 1, 8, p, None, None) == E
    assert lib.cds_mesh_cc_hook(p, 2 ** 31, 8, p, p, None) == E and lib.cds_mesh_cc_hook(None, 0, 8, None, None, None) == 0
    assert lib.cds_mesh_cc_jump(None, 8, None) == E
    assert lib.cds_mesh_cc_count(p, 1, 8, None, p, None) == E and lib.cds_mesh_cc_count(p, 1, 8, p, None, None) == E
    assert lib.cds_mesh_cc_mark(p, 1, 8, p, None, p, p, None) == E and lib.cds_mesh_cc_mark(p, 1, 8, p, p, p, None, None) == E
    assert lib.cds_mesh_cc_gather(p, None, p, 8, 1, p, p, p, p, 9, 1, p, None, p, None) == E        # more out than in
    assert lib.cds_mesh_cc_gather(p, None, p, 8, 1, p, p, p, p, 3, 2, p, None, p, None) == E
    assert lib.cds_mesh_cc_gather(None, None, p, 8, 1, p, p, p, p, 3, 1, p, None, p, None) == E
    assert lib.cds_mesh_cc_gather(p, p, p, 8, 1, p, p, p, p, 3, 1, p, None, p, None) == E           # colours in, nowhere to put them
    assert lib.cds_mesh_cc_gather(None, None, None, 8, 1, None, None, None, None, 0, 0, None, None, None, None) == 0
    torch.cuda.synchronize()


SENTINEL = 0xA5                                                          # every byte of an output before a gather


def _gather_case(case):
    """-> (vertex bits uint32 [V,3], colours uint8 [V,3], faces int32 [F,3], vertex keep uint8 [V], face keep uint8 [F]).  "a": the
    8 vertices and six faces of test_entry_points_skip_what_the_wrapper_never_sends, all flagged kept; "b": 257 vertices and 300
    random faces with three faces outside the vertices put in, random flags: the first face item is thread 1 of the second of
    three workgroups.  A vertex is kept iff a kept face inside the vertices holds it."""
    rng = np.random.default_rng(17)
    if case == "a":
        nv = 8
        faces = np.array([[0, 1, 2], [7, 8, 1], [4, 5, 6], [-1, 0, 4], [2, 3, 3], [0, 4, 2 ** 31 - 1]], np.int32)
        fkeep = np.ones(len(faces), np.uint8)
    else:
        nv = 257
        faces = rng.integers(0, nv, (303, 3)).astype(np.int32)
        faces[[5, 256, 302]] = [[3, nv, 9], [-1, 0, 4], [0, 4, 2 ** 31 - 1]]
        fkeep = rng.integers(0, 2, len(faces)).astype(np.uint8)
        fkeep[[5, 302]] = 1                                                # flagged and outside the vertices: skipped all the same
    inside = ((faces >= 0) & (faces < nv)).all(1)
    assert (~inside).sum() == 3
    vkeep = np.zeros(nv, np.uint8)
    vkeep[faces[inside & (fkeep != 0)].reshape(-1)] = 1
    assert 0 < vkeep.sum() < nv and 0 < fkeep.sum()
    bits = rng.normal(size=(nv, 3)).astype(np.float32).view(np.uint32).copy()
    bits[np.nonzero(vkeep)[0][0]] = [0x80000000, 0x7f800000, 0xffc12345]   # -0.0, an infinity, a NaN with a payload
    return bits, rng.integers(0, 256, (nv, 3)).astype(np.uint8), faces, vkeep, fkeep


def _numpy_gather(bits, col, faces, vkeep, fkeep):
    """The compaction in numpy, into arrays of the input's size filled with the sentinel -> (vertex bits, colours, faces, kept
    vertices, kept flags of faces, vertex_new, face_new)."""
    nv, nf = len(bits), len(faces)
    vnew = (np.cumsum(vkeep) - vkeep).astype(np.int32)
    fnew = (np.cumsum(fkeep) - fkeep).astype(np.int32)
    want_v = np.full((nv, 3), SENTINEL * 0x01010101, np.uint32)
    want_c = np.full((nv, 3), SENTINEL, np.uint8)
    want_f = np.full((nf, 3), SENTINEL, np.uint8).repeat(4, 1).view(np.int32)
    kept = np.nonzero(vkeep)[0]
    want_v[:len(kept)], want_c[:len(kept)] = bits[kept], col[kept]
    for f in np.nonzero(fkeep)[0]:
        if (faces[f] >= 0).all() and (faces[f] < nv).all():               # else the row of this face keeps the sentinel
            want_f[fnew[f]] = vnew[faces[f]]
    return want_v, want_c, want_f, len(kept), int(fkeep.sum()), vnew, fnew


@pytest.mark.parametrize("case", ["a", "b"])
def test_the_two_gathers_are_one_rule(case):
    """cds_mesh_cc_gather with byte colours and cds_mesh_simplify_gather with the packed words of the same colours (positions =
    vertices, face_clusters = faces, n_clusters = n_vertices) write the same bytes, those of a numpy gather; the rows of the
    flagged faces outside the vertices, and everything behind the kept rows, keep the sentinel.  The same without colours."""
    from cds_mvsnet_amd.pointcloud import pack_colors
    lib = _lib.load()
    bits, col, faces, vkeep, fkeep = _gather_case(case)
    want_v, want_c, want_f, nv_out, nf_out, vnew, fnew = _numpy_gather(bits, col, faces, vkeep, fkeep)
    nv, nf = len(bits), len(faces)
    skipped = [int(fnew[f]) for f in np.nonzero(fkeep)[0] if not ((faces[f] >= 0) & (faces[f] < nv)).all()]
    assert skipped and (want_f[skipped].view(np.uint8) == SENTINEL).all() and (want_f[nf_out:].view(np.uint8) == SENTINEL).all()
    tv, tc, tf = torch.from_numpy(bits.view(np.float32)).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(faces).cuda()
    assert np.array_equal(tv.cpu().numpy().view(np.uint32), bits)        # the upload kept the NaN's payload
    packed = pack_colors(tc)
    tvk, tfk = torch.from_numpy(vkeep).cuda(), torch.from_numpy(fkeep).cuda()
    tvn, tfn = torch.from_numpy(vnew).cuda(), torch.from_numpy(fnew).cuda()
    for with_colors in (True, False):
        got = {}
        for name in ("cc", "simplify"):
            ov = torch.full((nv, 3), SENTINEL, dtype=torch.uint8, device="cuda").repeat_interleave(4, 1).view(torch.float32)
            oc = torch.full((nv, 3), SENTINEL, dtype=torch.uint8, device="cuda")
            of = torch.full((nf, 3), SENTINEL, dtype=torch.uint8, device="cuda").repeat_interleave(4, 1).view(torch.int32)
            tail = (tvk.data_ptr(), tvn.data_ptr()), (tfk.data_ptr(), tfn.data_ptr(), nv_out, nf_out, ov.data_ptr(),
                                                      oc.data_ptr() if with_colors else None, of.data_ptr(), None)
            if name == "cc":
                rc = lib.cds_mesh_cc_gather(tv.data_ptr(), tc.data_ptr() if with_colors else None, tf.data_ptr(), nv, nf, *tail[0],
                                            *tail[1])
            else:
                rc = lib.cds_mesh_simplify_gather(tv.data_ptr(), packed.data_ptr() if with_colors else None, nv, *tail[0],
                                                  tf.data_ptr(), nf, *tail[1])
            assert rc == 0, f"{name}: {rc}"
            torch.cuda.synchronize()
            got[name] = (ov.cpu().numpy().view(np.uint32), oc.cpu().numpy(), of.cpu().numpy())
        for k, (what, want) in enumerate((("vertices", want_v), ("colors", want_c if with_colors else np.full_like(want_c, SENTINEL)),
                                          ("faces", want_f))):
            _same(got["cc"][k], got["simplify"][k], f"case {case}, colours {with_colors}: {what} of the two entry points")
            _same(got["cc"][k], want, f"case {case}, colours {with_colors}: {what} against numpy")


def test_two_runs_are_equal():
    f = torch.from_numpy(C.strip(1 << 16, "random", seed=5)).cuda()
    a, b = mesh.mesh_components(f, 1 << 16), mesh.mesh_components(f, 1 << 16)
    assert torch.equal(a["label"], b["label"]) and torch.equal(a["faces"], b["faces"])


# -------------------------------------------------------------------------------------------------------------- end to end
def _threshold(path):
    """A saved mesh -> (its arrays, N): N is the face count of its largest component when a smaller one with faces exists (so
    that something goes and something stays), else None."""
    v, c, f = mesh.read_mesh_ply(path)
    counts = C.components(f, len(v))["faces"]
    counts = counts[counts > 0]
    n = int(counts.max()) if len(counts) > 1 and counts.min() < counts.max() else None
    print(f"{os.path.basename(path)}: {len(f)} faces in {len(counts)} components, the largest {counts.max() if len(counts) else 0}")
    return (v, c, f), n


def _expected_file(tmp_path, arrays, name, **kw):
    out, info = C.clean(*arrays, **kw)
    path = str(tmp_path / name)
    mesh.write_mesh_ply(path, out["vertices"], out["colors"], out["faces"])
    return open(path, "rb").read(), info


def test_mesh_scan_and_command_line(tmp_path, capsys, monkeypatch):
    """The synthetic scan of test_mesh_gpu (3 views of 24 x 40): the file written with a threshold is clean_mesh of the file
    written without one, through mesh_scan, mesh.main and a child process; options at 0 change no byte and launch nothing;
    --from_mesh cleans a saved file in place."""
    scan, pairs = _write_outputs(tmp_path)
    out = tmp_path / "out"
    kw = dict(thres_view=1)
    plain = str(tmp_path / "plain_mesh.ply")
    info0 = mesh.mesh_scan(str(pairs), str(scan), plain, VOXEL, **kw)
    arrays, n = _threshold(plain)
    assert len(arrays[2]) > 0
    # options at 0: the same bytes, the same fields, the same line, and no clean-up kernel
    def no_clean(*a, **k):
        raise AssertionError("clean_mesh ran with both options at 0")
    zero = str(tmp_path / "zero_mesh.ply")
    with monkeypatch.context() as mp:
        mp.setattr(mesh, "clean_mesh", no_clean)
        info = mesh.mesh_scan(str(pairs), str(scan), zero, VOXEL, min_component=0, keep_largest=0, **kw)
    assert filecmp.cmp(plain, zero, shallow=False) and sorted(info) == sorted(info0) == ["blocks", "cloud", "faces", "mesh", "vertices"]
    assert mesh.format_mesh(info) == mesh.format_mesh(info0) == f"{info0['vertices']} vertices, {info0['faces']} faces, {info0['blocks']} blocks"
    cli = ["--testpath", str(tmp_path / "in"), "--outdir", str(out), "--testlist", str(tmp_path / "list.txt"), "--thres_view", "1",
           "--mesh_voxel", str(VOXEL)]
    mesh.main(cli)
    absent = open(out / "scan1_mesh.ply", "rb").read()
    mesh.main(cli + ["--mesh_min_component", "0", "--mesh_keep_largest", "0"])
    assert open(out / "scan1_mesh.ply", "rb").read() == absent == open(plain, "rb").read()
    # a threshold from the mesh's own counts, when it has more than one size of component; else the mesh is one piece and every
    # N up to its size keeps it
    nn = n if n is not None else len(arrays[2])
    want, winfo = _expected_file(tmp_path, arrays, "want.ply", min_faces=nn)
    direct = str(tmp_path / "direct_mesh.ply")
    info = mesh.mesh_scan(str(pairs), str(scan), direct, VOXEL, min_component=nn, **kw)
    assert open(direct, "rb").read() == want
    assert info["faces"] == winfo["faces"][1] > 0 and info["clean"]["faces"] == winfo["faces"] and info["blocks"] == info0["blocks"]
    assert (n is None) == (winfo["faces"][0] == winfo["faces"][1])
    assert torch.equal(info["mesh"]["faces"].cpu(), torch.from_numpy(mesh.read_mesh_ply(direct)[2]))     # what render_scan gets
    capsys.readouterr()
    assert mesh.main(cli + ["--mesh_min_component", str(nn)])["scan1"]["faces"] == winfo["faces"][1]
    line = capsys.readouterr().out
    assert f"removed {winfo['components'][0] - winfo['components'][1]} of {winfo['components'][0]} components" in line
    assert open(out / "scan1_mesh.ply", "rb").read() == want
    os.remove(out / "scan1_mesh.ply")
    stdout = _child("cds_mvsnet_amd.mesh", cli + ["--mesh_min_component", str(nn), "--mesh_keep_largest", "1"])
    assert open(out / "scan1_mesh.ply", "rb").read() == _expected_file(tmp_path, arrays, "want1.ply", min_faces=nn, keep_largest=1)[0]
    assert "scan1_mesh.ply:" in stdout and "components" in stdout
    # --from_mesh: debris appended to the saved file (two tetrahedra and a vertex in no face), cleaned in place, no --testpath
    v, c, f = arrays
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    v2 = np.concatenate([corner + 5000, v, corner - 5000, np.zeros((1, 3), np.float32)]).astype(np.float32)
    c2 = np.concatenate([np.full((4, 3), 9, np.uint8), c, np.full((5, 3), 200, np.uint8)])
    f2 = np.concatenate([C.TETRA, f + 4, C.TETRA + 4 + len(v)]).astype(np.int32)
    saved = str(out / "scan1_mesh.ply")
    mesh.write_mesh_ply(saved, v2, c2, f2)
    want5, info5 = _expected_file(tmp_path, (v2, c2, f2), "want5.ply", min_faces=5)
    assert info5["faces"][1] < info5["faces"][0] and info5["faces"][1] > 0          # something goes and something stays
    res = mesh.main(["--from_mesh", str(out / "{scan}_mesh.ply"), "--mesh_min_component", "5", "--outdir", str(out), "--testlist",
                     str(tmp_path / "list.txt")])
    assert open(saved, "rb").read() == want5 and res["scan1"]["clean"]["faces"] == info5["faces"]
    assert "blocks" not in capsys.readouterr().out
    _check_file(saved)


@pytest.fixture(scope="module")
def plain_infer(tmp_path_factory):
    """infer --fuse --mesh_voxel 10 without the new options on a scene of test_mvs_io._write_scene (3 views of 128 x 160, an
    untrained network, the loose settings of test_mesh_gpu.test_infer_fuse_mesh) -> (root, list, base arguments, output folder)."""
    tmp = tmp_path_factory.mktemp("clean_infer")
    root = str(tmp / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanA", 3, 128, 160, seed=3)
    lst = str(tmp / "list.txt")
    with open(lst, "w") as f:
        f.write("scanA\n")
    base = ["--testpath", root, "--testlist", lst, "--num_view", "3", "--max_h", "128", "--max_w", "160", "--interval_scale", "1.0",
            "--fuse", "--mesh_voxel", "10"] + FUSE
    plain = str(tmp / "plain")
    infer.main(base + ["--outdir", plain])
    return tmp, root, base, plain


def test_infer_options_at_zero_change_no_file(plain_infer):
    tmp, root, base, plain = plain_infer
    zero = str(tmp / "zero")
    infer.main(base + ["--outdir", zero, "--mesh_min_component", "0", "--mesh_keep_largest", "0"])
    assert _tree(plain) == _tree(zero) and "scanA_mesh.ply" in _tree(plain)
    for name in _tree(plain):
        assert filecmp.cmp(os.path.join(plain, name), os.path.join(zero, name), shallow=False), name


def test_infer_clean_and_render(plain_infer, tmp_path, capsys):
    """infer --fuse --mesh_voxel --mesh_min_component N --render_mesh: the mesh file is clean_mesh of the file of the run without
    the option, and depth_mesh is render_scan of that cleaned mesh."""
    tmp, root, base, plain = plain_infer
    arrays, n = _threshold(os.path.join(plain, "scanA_mesh.ply"))
    assert n is not None, "the scene's mesh is one piece: this test needs debris"
    want, winfo = _expected_file(tmp_path, arrays, "want.ply", min_faces=n)
    assert 0 < winfo["faces"][1] < winfo["faces"][0]
    out = str(tmp / "clean")
    capsys.readouterr()
    infer.main(base + ["--outdir", out, "--mesh_min_component", str(n), "--render_mesh"])
    lines = capsys.readouterr().out.splitlines()
    assert open(os.path.join(out, "scanA_mesh.ply"), "rb").read() == want
    line = [ln for ln in lines if "scanA_mesh.ply" in ln]
    assert line and f"{winfo['faces'][1]} faces" in line[0] and f"{winfo['faces'][0] - winfo['faces'][1]} of {winfo['faces'][0]} faces" in line[0]
    # every other file of the scan is the file of the plain run; depth_mesh is the render of the cleaned file
    for name in _tree(plain):
        if name != "scanA_mesh.ply":
            assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    scan = os.path.join(out, "scanA")
    render.render_scan(scan, os.path.join(out, "scanA_mesh.ply"), os.path.join(root, "scanA"), subdir="again")
    render.render_scan(scan, os.path.join(plain, "scanA_mesh.ply"), os.path.join(root, "scanA"), subdir="dirty")
    differ = 0
    for i in range(3):
        a = mvs_io.read_pfm(os.path.join(scan, "depth_mesh", f"{i:08d}.pfm"))[0]
        b = mvs_io.read_pfm(os.path.join(scan, "again", f"{i:08d}.pfm"))[0]
        d = mvs_io.read_pfm(os.path.join(scan, "dirty", f"{i:08d}.pfm"))[0]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (a > 0).any()
        differ += int((a.view(np.uint32) != d.view(np.uint32)).sum())
    print(f"N = {n}: {winfo['faces'][0]} -> {winfo['faces'][1]} faces; {differ} pixels of depth_mesh change")
