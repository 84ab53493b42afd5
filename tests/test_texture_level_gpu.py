"""The seam-levelling kernels of csrc/mesh_texture.hip against the numpy restatement of rules L1-L6 (texture_level_ref.py, DESIGN
§1.19): nodes, samples, pair table, g and atlas equal in every bit, the offsets within the solver's bound; what does not change
without the option; refusals; and the way through infer, the texture command line and photo_eval."""
import filecmp
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_ref as R
import texture_level_ref as L
import texture_ref as T
from cds_mvsnet_amd import infer, photo_eval, texture
from test_mvs_io import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atlas", "uv", "view", "cell")
LEVEL = ("node_key", "corner_node", "sample", "ok", "offsets", "g")
DTYPES = dict(node_key=np.int64, corner_node=np.int32, sample=np.float64, ok=np.uint8, offsets=np.float64, g=np.float64)


def _mesh(v, c, f):
    return {"vertices": torch.from_numpy(v).cuda(), "colors": torch.from_numpy(c).cuda(), "faces": torch.from_numpy(f).cuda()}


def _gpu(v, c, f, images, cams, **kw):
    """-> (the four arrays, the arrays of "level" or None, info)."""
    if isinstance(images, list):
        out, info = texture.texture_mesh(_mesh(v, c, f), [torch.from_numpy(i).cuda() for i in images], [torch.from_numpy(k) for k in cams], **kw)
    else:
        out, info = texture.texture_mesh(_mesh(v, c, f), torch.from_numpy(images).cuda(), torch.from_numpy(cams), **kw)
    lv = out.pop("level", None)
    assert sorted(out) == sorted(NAMES) and all(t.is_cuda for t in out.values())
    if lv is not None:
        assert sorted(lv) == sorted(LEVEL) and all(t.is_cuda for t in lv.values())
        lv = {k: t.cpu().numpy() for k, t in lv.items()}
        assert all(lv[k].dtype == DTYPES[k] for k in LEVEL)
    return {k: t.cpu().numpy() for k, t in out.items()}, lv, info


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {a.shape}, expected {b.dtype} {b.shape}"
    bad = a.view(np.uint64) != b.view(np.uint64) if a.dtype == np.float64 else a != b
    assert not bad.any(), f"{what} differs in {int(bad.sum())} of {bad.size} places, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"{a[tuple(np.argwhere(bad)[0])]!r} for {b[tuple(np.argwhere(bad)[0])]!r}"


def _offset_bound(table, node_key, n_views):
    want, M = L.offsets_lstsq(table, node_key, n_views)
    return np.linalg.cond(M.T @ M) * 2.0 ** -50 * np.abs(want).max()


def _check(v, c, f, images, cams, iters=(7,), lam=0.1, what="", base=None, **kw):
    """The library at every ITER of ``iters`` against the restatement run from the library's offsets; the unlevelled call.
    base: the restatement's unlevelled result, where texture_ref has it at hand."""
    plain, none, _ = _gpu(v, c, f, images, cams, **kw)
    assert none is None
    tex = {k: kw[k] for k in ("scale", "max_cell", "min_px") if k in kw}
    base = base if base is not None else T.texture(v, c, f, images, cams, **tex)
    got = {it: _gpu(v, c, f, images, cams, level=it, level_lambda=lam, **kw) for it in iters}
    first = got[iters[0]][1]
    want = L.level(v, c, f, images, cams, max(iters), lam, base=base, force_offsets=first["offsets"], keep=iters)
    lv = want["level"]
    n_views = len(first["offsets"])
    for it in iters:
        out, mine, info = got[it]
        for k in ("uv", "view", "cell"):
            _bits(out[k], plain[k], f"{what} level {it}: {k} against the unlevelled call")
        for k in ("node_key", "corner_node", "ok"):
            _bits(mine[k], lv[k], f"{what} level {it}: {k}")
        _bits(mine["sample"], lv["sample"], f"{what} level {it}: sample")
        _bits(mine["offsets"], first["offsets"], f"{what} level {it}: offsets, run to run")
        _bits(mine["g"], lv["g_at"][it], f"{what}: g after {it} iterations")
        pairs, before = L.seam_jump(lv["sample"], lv["ok"], lv["node_key"], n_views, np.zeros_like(lv["g"]))
        _, after = L.seam_jump(lv["sample"], lv["ok"], lv["node_key"], n_views, lv["g_at"][it])
        assert info["seam"][0] == pairs and np.allclose(info["seam"][1:], (before, after), rtol=1e-9, atol=1e-9), (info["seam"], pairs, before, after)
    last = max(iters)
    _bits(got[last][0]["atlas"], want["atlas"], f"{what} level {last}: atlas")
    # the pair table, and the offsets against the restatement's own
    t = {k: torch.from_numpy(first[k]).cuda() for k in ("node_key", "sample", "ok")}
    table = texture.level_pair_table(t["node_key"], t["sample"], t["ok"], n_views)[0].cpu().numpy()
    _bits(table, lv["table"], f"{what}: pair table")
    mine_o = L.offsets(lv["table"], lv["node_key"], n_views)
    err = float(np.abs(first["offsets"] - mine_o).max()) if n_views else 0.0
    bound = _offset_bound(lv["table"], lv["node_key"], n_views)
    print(f"{what}: {len(lv['node_key'])} nodes, {int(lv['table'][:, :, 0].sum())} seam pairs, {int((got[last][0]['atlas'] != plain['atlas']).any(2).sum())} "
          f"texels changed, seam {got[last][2]['seam']}, offsets off by {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    return got[last], plain, want


# --------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name,n_views", [("plane", 3), ("sphere", 3), ("sphere", 9), ("wild", 3), ("clutter", 3)])
def test_kernels_equal_the_restatement(name, n_views):
    (out, lv, info), plain, want = _check(*T.case(name, n_views), iters=(1, 2, 7), what=f"{name} {n_views}", base=T.reference(name, n_views))
    assert (plain["view"] >= 0).any() and len(lv["node_key"]) > 0
    if name != "clutter":
        assert info["seam"][0] > 0 and (out["atlas"] != plain["atlas"]).any()
    else:
        assert info["seam"] == (0, 0.0, 0.0) and not lv["g"].any() and np.array_equal(out["atlas"], plain["atlas"])


def test_exposure_steps_are_levelled_on_the_gpu():
    """The plane of DESIGN §1.19 with +0 / +25 / -20 levels per view: the library's atlas is the restatement's."""
    v, vc, f, images, shifted, cams = L.plane_setup()
    (out, lv, info), plain, want = _check(v, vc, f, shifted, cams, iters=(20,), what="exposure plane")
    assert info["seam"][0] == 31 and info["seam"][2] <= 0.1 * info["seam"][1]
    assert L.pattern_rms(v, f, out) <= 0.25 * L.pattern_rms(v, f, plain)


# ------------------------------------------------------------------------------------------------ invariance, repeatability
def test_level_zero_is_todays_call_and_runs_repeat():
    case = T.case("sphere", 9)
    plain, none, info = _gpu(*case)
    zero, lv0, info0 = _gpu(*case, level=0, level_lambda=0.5)
    assert none is None and lv0 is None and "seam" not in info and info0 == info
    for k in NAMES:
        _bits(zero[k], plain[k], f"level 0: {k}")
        _bits(plain[k], T.reference("sphere", 9)[k], f"unlevelled: {k}")
    a, la, ia = _gpu(*case, level=7)
    b, lb, ib = _gpu(*case, level=7)
    assert ia == ib
    for k in NAMES:
        _bits(b[k], a[k], f"second run: {k}")
    for k in LEVEL:
        _bits(lb[k], la[k], f"second run: {k}")
    for chunk in (1, 8, 32):
        c, lc, _ = _gpu(*case, level=7, chunk=chunk)
        _bits(c["atlas"], a["atlas"], f"chunk {chunk}: atlas")
        for k in LEVEL:
            _bits(lc[k], la[k], f"chunk {chunk}: {k}")


def test_both_forms_of_the_fill_give_the_same(monkeypatch):
    case = T.case("sphere", 3)
    a, la, _ = _gpu(*case, level=7, scale=8.0, max_cell=16)
    monkeypatch.setattr(texture, "FILL_PER_UNIT", 1 - texture.FILL_PER_UNIT)
    b, lb, _ = _gpu(*case, level=7, scale=8.0, max_cell=16)
    _bits(b["atlas"], a["atlas"], "the other fill")


# --------------------------------------------------------------------------------------------------------------- edge cases
def test_views_of_two_image_sizes_in_both_orders():
    v, c, f, images, _ = T.case("sphere", 3)
    cams, small = R.view_cameras(5), T.view_images(2, 37, 50, seed=5)
    (out, lv, info), plain, _ = _check(v, c, f, [images, small], [cams[:3], cams[3:]], what="two sizes")
    assert set(np.unique(plain["view"]).tolist()) == {-1, 0, 1, 2, 3, 4} and info["seam"][0] > 0
    _check(v, c, f, [small, images], [cams[3:], cams[:3]], what="small first")
    _check(v, c, f, [images, small], [cams[:3], cams[3:]], what="two sizes, chunk 2", chunk=2)


def test_map_of_50_by_37():
    _check(*T.case("wild", 2, 37, 50), what="wild 50 x 37", base=T.reference("wild", 2, 37, 50))
    _check(*T.case("sphere", 2, 37, 50), what="sphere 50 x 37", base=T.reference("sphere", 2, 37, 50))


def test_image_one_pixel_wide():
    (out, lv, info), plain, _ = _check(*T.case("special", 1, R.H, 1), what="one pixel wide", base=T.reference("special", 1, R.H, 1))
    assert plain["view"][0] == 0 and lv["ok"].any()


def test_cells_of_four_texels():
    """scale 0.25 at max_cell 16: every cell has c = 4, so wa, wb, wc extrapolate into the gutter with weights up to 1.25."""
    (out, lv, info), plain, _ = _check(*T.case("sphere", 3), scale=0.25, max_cell=16, what="cells of 4",
                                       base=T.reference("sphere", 3, R.H, R.W, 0.25, 16))
    assert set(np.unique(plain["cell"][:, 2]).tolist()) == {4} and (out["atlas"] != plain["atlas"]).any()


def test_two_identical_cameras():
    v, c, f, images, _ = T.case("sphere", 2)
    cams = R.view_cameras(1).repeat(2, 0)
    (out, lv, info), plain, _ = _check(v, c, f, images, cams, what="identical cameras")
    assert set(np.unique(plain["view"]).tolist()) == {-1, 0} and info["seam"] == (0, 0.0, 0.0) and not lv["g"].any()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_entry_points_refuse_what_the_wrapper_never_sends():
    lib, E = texture._lib.load(), texture._lib.EINVAL
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    u = torch.zeros(64, dtype=torch.int64, device="cuda")
    p, q = t.data_ptr(), u.data_ptr()
    big = 2 ** 31
    samples = lambda **k: lib.cds_texture_level_samples(k.get("vertices", p), k.get("nv", 4), p, p, k.get("image_bytes", 48), k.get("views", p),
                                                       k.get("n_views", 1), k.get("node_key", p), k.get("n", 4), k.get("sample", p), k.get("ok", p), None)
    for bad in (dict(vertices=None), dict(nv=-1), dict(nv=big), dict(image_bytes=-1), dict(views=None), dict(n_views=0), dict(n_views=513),
                dict(node_key=None), dict(n=-1), dict(n=big), dict(sample=None), dict(ok=None)):
        assert samples(**bad) == E, bad
    pairs = lambda **k: lib.cds_texture_level_pairs(k.get("sample", p), k.get("ok", p), k.get("node_key", p), k.get("span", p), k.get("n", 4),
                                                   k.get("n_views", 2), k.get("table", p), None)
    for bad in (dict(sample=None), dict(ok=None), dict(node_key=None), dict(span=None), dict(n=-1), dict(n=big), dict(n_views=0),
                dict(n_views=513), dict(table=None)):
        assert pairs(**bad) == E, bad
    step = lambda **k: lib.cds_texture_level_step(k.get("sample", p), p, k.get("span", p), k.get("start", p), k.get("clist", p), k.get("n_list", 8), k.get("cnode", p),
                                                 k.get("n", 4), k.get("nf", 4), k.get("n_views", 2), k.get("lam", 0.1), k.get("g_in", p),
                                                 k.get("g_out", q), None)
    for bad in (dict(sample=None), dict(span=None), dict(start=None), dict(clist=None), dict(cnode=None), dict(n=-1), dict(n=big), dict(nf=-1),
                dict(n_list=-1), dict(n_list=13), dict(n_views=0), dict(n_views=513), dict(lam=0.0), dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")),
                dict(g_in=None), dict(g_out=None), dict(g_out=p)):
        assert step(**bad) == E, bad
    fill = lambda **k: lib.cds_texture_fill_level(p, p, 4, p, 4, p, p, k.get("image_bytes", 48), k.get("views", p), k.get("n_views", 1), p, p,
                                                 p, p, k.get("total", 1), 16, k.get("ah", 4), k.get("aw", 4), k.get("atlas", p),
                                                 k.get("per_unit", 0), k.get("cnode", p), k.get("g", p), k.get("n", 4), None)
    for bad in (dict(image_bytes=-1), dict(views=None), dict(n_views=0), dict(total=2), dict(aw=12, ah=12), dict(atlas=None), dict(atlas=p + 1),
                dict(per_unit=2), dict(cnode=None), dict(g=None), dict(n=-1), dict(n=big)):
        assert fill(**bad) == E, bad
    # zero nodes: nothing to do, before any pointer is looked at
    assert samples(n=0, sample=None) == 0 and pairs(n=0, table=None) == 0 and step(n=0, g_in=None) == 0
    torch.cuda.synchronize()
    assert int(t.abs().sum()) == 0 and int(u.abs().sum()) == 0          # nothing was written


def _tables(v, c, f, images, cams, level=3):
    """The device tensors texture_mesh works on, for direct calls of the entry points."""
    m = _mesh(v, c, f)
    ti = torch.from_numpy(images).cuda()
    out, info = texture.texture_mesh(m, ti, torch.from_numpy(cams), level=level)
    n, h, w = images.shape[:3]
    views = torch.tensor([(3 * h * w * k, h, w) for k in range(n)], dtype=torch.int64).cuda()
    tab = texture.camera_table(torch.from_numpy(cams)).cuda()
    return m, ti, views, tab, out, info


def test_view_entry_outside_the_bytes_makes_its_nodes_not_ok():
    v, c, f, images, cams = T.case("sphere", 3)
    m, ti, views, tab, out, _ = _tables(v, c, f, images, cams)
    lib, lv = texture._lib.load(), out["level"]
    n, nbytes = int(lv["node_key"].numel()), int(ti.numel())
    label = (lv["node_key"] % 3).cpu().numpy()
    assert (label == 1).any() and lv["ok"].cpu().numpy()[label == 1].all()
    for entry in ((nbytes - 3 * 64 * 48 + 1, 48, 64), (-1, 48, 64), (0, 0, 64), (0, 48, 2 ** 40)):
        bad = views.clone()
        bad[1] = torch.tensor(entry, dtype=torch.int64, device="cuda")
        sample = torch.full((n, 3), -1.0, dtype=torch.float64, device="cuda")
        ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        assert lib.cds_texture_level_samples(m["vertices"].data_ptr(), len(v), tab.data_ptr(), ti.data_ptr(), nbytes, bad.data_ptr(), 3,
                                             lv["node_key"].data_ptr(), n, sample.data_ptr(), ok.data_ptr(), None) == 0
        s, o = sample.cpu().numpy(), ok.cpu().numpy()
        assert not o[label == 1].any() and not s[label == 1].any(), entry
        _bits(s[label != 1], lv["sample"].cpu().numpy()[label != 1], f"{entry}: the other views' samples")
        _bits(o[label != 1], lv["ok"].cpu().numpy()[label != 1], f"{entry}: the other views' ok")
    # keys that no mesh gives: negative, and a vertex outside the vertices
    keys = torch.tensor([-1, -3 * 10 ** 9, 3 * len(v), 3 * len(v) + 2, 2 ** 62], dtype=torch.int64, device="cuda")
    sample = torch.full((5, 3), -1.0, dtype=torch.float64, device="cuda")
    ok = torch.full((5,), 7, dtype=torch.uint8, device="cuda")
    assert lib.cds_texture_level_samples(m["vertices"].data_ptr(), len(v), tab.data_ptr(), ti.data_ptr(), nbytes, views.data_ptr(), 3,
                                         keys.data_ptr(), 5, sample.data_ptr(), ok.data_ptr(), None) == 0
    assert not ok.cpu().numpy().any() and not sample.cpu().numpy().any()


def test_corner_nodes_outside_the_nodes_leave_their_faces_unlevelled():
    v, c, f, images, cams = T.case("sphere", 3)
    m, ti, views, tab, out, info = _tables(v, c, f, images, cams, level=7)
    plain, _ = texture.texture_mesh(m, ti, torch.from_numpy(cams))
    lib, lv = texture._lib.load(), out["level"]
    n, nf = int(lv["node_key"].numel()), len(f)
    size = out["cell"][:, 2].to(torch.int64)
    order = torch.sort(-size, stable=True).indices
    units = (size[order] >> 2) ** 2
    ends = torch.cumsum(units, 0)
    starts, total = ends - units, int(ends[-1])
    H, W = out["atlas"].shape[:2]
    seen = np.nonzero(out["view"].cpu().numpy() >= 0)[0]
    hit = {int(seen[0]): -1, int(seen[5]): n, int(seen[11]): 2 ** 31 - 1, int(seen[17]): -(2 ** 31)}
    cn = lv["corner_node"].clone()
    for k, (face, value) in enumerate(hit.items()):
        cn[face, k % 3] = value
    for per_unit in (0, 1):
        atlas = torch.full((H, W, 3), 99, dtype=torch.uint8, device="cuda")
        args = (m["vertices"].data_ptr(), m["colors"].data_ptr(), len(v), m["faces"].data_ptr(), nf, tab.data_ptr(), ti.data_ptr(),
                int(ti.numel()), views.data_ptr(), 3, out["view"].data_ptr(), out["cell"].data_ptr(), order.data_ptr(), starts.data_ptr(),
                total, 256, H, W, atlas.data_ptr(), per_unit)
        assert lib.cds_texture_fill_level(*args, cn.data_ptr(), lv["g"].data_ptr(), n, None) == 0
        got, levelled, unlevelled = atlas.cpu().numpy(), out["atlas"].cpu().numpy(), plain["atlas"].cpu().numpy()
        want = levelled.copy()
        changed = 0
        for face in hit:
            x0, y0, cc = out["cell"][face].cpu().tolist()
            want[y0:y0 + cc, x0:x0 + cc] = unlevelled[y0:y0 + cc, x0:x0 + cc]
            changed += int((levelled[y0:y0 + cc, x0:x0 + cc] != unlevelled[y0:y0 + cc, x0:x0 + cc]).sum())
        assert changed > 0
        _bits(got, want, f"per_unit {per_unit}: atlas with four faces unlevelled")
        # zero nodes: every corner node is outside, the atlas is the unlevelled one
        assert lib.cds_texture_fill_level(*args, cn.data_ptr(), None, 0, None) == 0
        _bits(atlas.cpu().numpy(), unlevelled, f"per_unit {per_unit}: no nodes")


def test_step_skips_tables_that_do_not_fit():
    """Spans and corner lists that point outside their tables are not followed: such a node keeps what the rest of its tables
    give, and a node with neither keeps its g."""
    v, c, f, images, cams = T.case("sphere", 3)
    m, ti, views, tab, out, _ = _tables(v, c, f, images, cams, level=1)
    lib, lv = texture._lib.load(), out["level"]
    n, nf = int(lv["node_key"].numel()), len(f)
    table, span, _ = texture.level_pair_table(lv["node_key"], lv["sample"], lv["ok"], 3)
    flat = lv["corner_node"].reshape(-1)
    corners = torch.nonzero(flat >= 0).reshape(-1)
    corner_list = corners[torch.sort(flat[corners].to(torch.int64), stable=True).indices].contiguous()
    corner_start = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    corner_start[1:] = torch.cumsum(torch.bincount(flat[corners].to(torch.int64), minlength=n), 0)
    g0 = lv["offsets"][lv["node_key"] % 3].contiguous()

    def run(span, corner_start, corner_list, cnode):
        g1 = torch.full_like(g0, 12345.0)
        assert lib.cds_texture_level_step(lv["sample"].data_ptr(), lv["ok"].data_ptr(), span.data_ptr(), corner_start.data_ptr(),
                                          corner_list.data_ptr(), int(corner_list.numel()), cnode.data_ptr(), n, nf, 3, 0.1,
                                          g0.data_ptr(), g1.data_ptr(), None) == 0
        return g1.cpu().numpy()
    _bits(run(span, corner_start, corner_list, lv["corner_node"]), lv["g"].cpu().numpy(), "the tables of the wrapper")
    assert n > 8
    bad_span = span.cpu().clone()
    bad_span[:5] = torch.tensor([[-1, 2], [1, 4], [3, 1], [n - 1, 3], [4, 2 ** 31 - 1]], dtype=torch.int32)
    bad_span = bad_span.cuda()
    bad_start = torch.full_like(corner_start, 2 ** 40)
    bad_start[::2] = -7
    got = run(bad_span, bad_start, corner_list, lv["corner_node"])
    assert np.isfinite(got).all()
    _bits(got[:5], g0.cpu().numpy()[:5], "nodes without a usable table keep their g")
    bad_list = torch.full_like(corner_list, 3 * nf)
    bad_list[::2] = -1
    _bits(run(bad_span, corner_start, bad_list, lv["corner_node"])[:5], g0.cpu().numpy()[:5], "corners outside the faces")
    bad_node = torch.full_like(lv["corner_node"], n)
    bad_node[::2] = -1
    _bits(run(bad_span, corner_start, corner_list, bad_node)[:5], g0.cpu().numpy()[:5], "partners outside the nodes")
    # the pair table with such spans: skipped, never followed
    t2 = torch.zeros_like(table)
    wild = torch.stack([torch.full((n,), -5, dtype=torch.int32), torch.full((n,), 2 ** 31 - 1, dtype=torch.int32)], 1).cuda()
    assert lib.cds_texture_level_pairs(lv["sample"].data_ptr(), lv["ok"].data_ptr(), lv["node_key"].data_ptr(), wild.data_ptr(), n, 3,
                                       t2.data_ptr(), None) == 0
    assert int(t2.abs().sum()) == 0 and int(table[:, :, 0].sum()) > 0


# ------------------------------------------------------------------------------------------------------------- empty inputs
def test_empty_mesh_zero_views_and_cpu_tensors(monkeypatch):
    v, c, f, images, cams = T.case("plane", 2)
    m = _mesh(v, c, f)
    ti, tc = torch.from_numpy(images).cuda(), torch.from_numpy(cams)

    def no_launch():
        raise AssertionError("the library was loaded: a launch was about to happen")
    monkeypatch.setattr(texture._lib, "load", no_launch)
    monkeypatch.setattr(texture, "render_mesh", lambda *a, **k: no_launch())
    out, info = texture.texture_mesh(dict(m, faces=m["faces"][:0]), ti, tc, level=3)
    assert out["atlas"].shape == (0, 0, 3) and out["uv"].shape == (0, 3, 2) and info["H"] == 0 and info["seam"] == (0, 0.0, 0.0)
    assert out["level"]["corner_node"].shape == (0, 3) and out["level"]["g"].shape == (0, 3) and out["level"]["offsets"].shape == (2, 3)
    out, info = texture.texture_mesh(m, ti[:0], tc[:0], level=3)
    assert out["atlas"].shape == (0, 0, 3) and int((out["view"] != -1).sum()) == 0 and info["unseen"] == len(f)
    lv = out["level"]
    assert sorted(lv) == sorted(LEVEL) and all(t.is_cuda for t in lv.values()) and lv["node_key"].shape == (0,)
    assert lv["corner_node"].shape == (len(f), 3) and int((lv["corner_node"] != -1).sum()) == 0 and lv["offsets"].shape == (0, 3)
    assert {k: lv[k].dtype for k in LEVEL} == {k: getattr(torch, np.dtype(d).name) for k, d in DTYPES.items()}
    for bad in (dict(level=-1), dict(level=2, level_lambda=0.0)):
        with pytest.raises(ValueError, match="level"):
            texture.texture_mesh(m, ti, tc, **bad)
    for key in ("vertices", "colors", "faces"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            texture.texture_mesh(dict(m, **{key: m[key].cpu()}), ti, tc, level=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        texture.texture_mesh(m, ti.cpu(), tc, level=3)


def test_a_mesh_that_no_view_sees():
    (out, lv, info), plain, _ = _check(*T.case("unseen", 3), what="unseen", base=T.reference("unseen", 3))
    assert len(lv["node_key"]) == 0 and (lv["corner_node"] == -1).all() and info["seam"] == (0, 0.0, 0.0)
    assert np.array_equal(out["atlas"], plain["atlas"])


# ------------------------------------------------------------------------------------------------------------ end to end
FUSE = ["--filter_method", "dynamic", "--conf", "0.0,0.0,0.0", "--dyn_dist_base", "2.0", "--dyn_rel_base", "0.02", "--dyn_views", "1,10"]


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, n), root) for d, _, names in os.walk(root) for n in names)


def _equal(a, b):
    """Equality of JSON values in which a NaN equals a NaN."""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_infer_the_command_line_and_photo_eval(tmp_path, capsys):
    """infer --fuse --mesh_voxel --texture with and without --texture_level 5 on a scene of test_mvs_io._write_scene (3 views of
    128 x 160, an untrained network, loose consistency settings, as in test_texture_gpu), then the texture command line and
    photo_eval on the saved output."""
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanA", 3, 128, 160, seed=3)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("scanA\n")
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    base = ["--testpath", root, "--testlist", lst, "--num_view", "3", "--max_h", "128", "--max_w", "160", "--interval_scale", "1.0",
            "--fuse", "--mesh_voxel", "10", "--texture", "--texture_max_cell", "32"] + FUSE
    infer.main(base + ["--outdir", plain])
    assert not [ln for ln in capsys.readouterr().out.splitlines() if "seam pairs" in ln]
    infer.main(base + ["--outdir", out, "--texture_level", "5"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("scanA_textured.obj: atlas ")]
    assert len(lines) == 1 and "seam pairs levelled: mean jump " in lines[0], lines
    # the same files; all but the image are the same in every byte: the geometry, the UVs and everything before do not change
    names = _tree(plain)
    assert names == _tree(out) and "scanA_textured.png" in names and "scanA_textured.obj" in names
    for name in names:
        if name != "scanA_textured.png":
            assert filecmp.cmp(os.path.join(plain, name), os.path.join(out, name), shallow=False), name
    scan, ply, pairs = os.path.join(out, "scanA"), os.path.join(out, "scanA_mesh.ply"), os.path.join(root, "scanA")
    # the library call on the saved output: the PNG and the line of infer; level 0 and no keyword: the PNG of the plain run
    info = texture.texture_scan(scan, ply, pairs, str(tmp_path / "again"), max_cell=32, level=5)
    assert capsys.readouterr().out.splitlines() == [lines[0].replace("scanA_textured.obj", "again.obj")]
    assert info["seam"][0] > 0 and _read(str(tmp_path / "again.png")) == _read(os.path.join(out, "scanA_textured.png"))
    assert _read(os.path.join(out, "scanA_textured.png")) != _read(os.path.join(plain, "scanA_textured.png"))
    info0 = texture.texture_scan(scan, ply, pairs, str(tmp_path / "zero"), max_cell=32, level=0)
    assert "seam" not in info0 and _read(str(tmp_path / "zero.png")) == _read(os.path.join(plain, "scanA_textured.png"))
    capsys.readouterr()
    # the command line on the saved output reproduces the three files
    new = [f"scanA_textured.{e}" for e in ("mtl", "obj", "png")]
    saved = {n: _read(os.path.join(out, n)) for n in new}
    for n in new:
        os.remove(os.path.join(out, n))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "cds_mvsnet_amd.texture", "--testpath", root, "--outdir", out, "--testlist", lst,
                          "--texture_max_cell", "32", "--texture_level", "5"], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert lines[0] in res.stdout.splitlines()
    assert {n: _read(os.path.join(out, n)) for n in new} == saved
    # photo_eval: the JSON of the command line holds what the library call returns, and levelling reaches the score
    want = photo_eval.score_scan(scan, ply, pairs, max_cell=32, level=5)
    unlevelled = photo_eval.score_scan(scan, ply, pairs, max_cell=32)
    assert want["scored"] == 3 and want["psnr"] != unlevelled["psnr"]
    path = str(tmp_path / "scores.json")
    res = subprocess.run([sys.executable, "-m", "cds_mvsnet_amd.photo_eval", "--testpath", root, "--outdir", out, "--testlist", lst,
                          "--texture_max_cell", "32", "--texture_level", "5", "--json", path], env=env, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    with open(path) as f:
        got = json.load(f)
    assert _equal(got["scans"]["scanA"], json.loads(json.dumps(want)))
    assert got["settings"]["texture"]["level"] == 5 and got["settings"]["texture"]["level_lambda"] == 0.1
