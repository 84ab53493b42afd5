"""The host side of the texturing stage (cds_mvsnet_amd/texture.py) and the numpy restatement of its rule
(texture_ref.py): packing, UV, the view rule, the atlas size, the OBJ files, the command lines' errors, and what the feature is
for: a textured coarse mesh is closer to the surface's colour than its vertex colours."""
import numpy as np
import pytest
import torch

import render_ref as R
import texture_ref as T
from cds_mvsnet_amd import infer, texture


# ------------------------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("seed", range(20))
def test_packing_is_aligned_disjoint_and_inside_the_atlas(seed):
    rs = np.random.RandomState(seed)
    classes = rs.choice([4, 8, 16, 32, 64], size=rs.randint(1, 5), replace=False)
    c = rs.choice(classes, size=rs.randint(1, 400))
    order, starts, total, H, W, origin = T.pack(c)
    assert total == int(((c // 4) ** 2).sum()) and (H, W) == texture.atlas_size(total)
    assert W & (W - 1) == 0 and (W // 4) ** 2 >= total and (W == 4 or (W // 8) ** 2 < total)
    assert H == (W // 2 if 2 * total <= (W // 4) ** 2 else W)
    assert np.array_equal(c[order], np.sort(c)[::-1]) and all(order[k] < order[k + 1] for k in range(len(c) - 1) if c[order[k]] == c[order[k + 1]])
    taken = np.zeros((H, W), np.int32)
    for f in range(len(c)):
        x0, y0 = origin[f]
        assert x0 % c[f] == 0 and y0 % c[f] == 0 and x0 + c[f] <= W and y0 + c[f] <= H, (f, x0, y0, c[f])
        taken[y0:y0 + c[f], x0:x0 + c[f]] += 1
    assert taken.max() == 1 and int(taken.sum()) == 16 * total
    # the UV corners lie at least one texel inside their own cell
    uv = T.corner_uv(origin, c)
    for k in range(3):
        assert ((uv[:, k, 0] >= origin[:, 0] + 1) & (uv[:, k, 0] <= origin[:, 0] + c - 1)).all()
        assert ((uv[:, k, 1] >= origin[:, 1] + 1) & (uv[:, k, 1] <= origin[:, 1] + c - 1)).all()


def test_atlas_height_is_half_the_width_exactly_when_the_cells_fit_half():
    assert texture.atlas_size(1) == (4, 4)
    assert texture.atlas_size(2) == (4, 8) and texture.atlas_size(3) == (8, 8) and texture.atlas_size(4) == (8, 8)
    assert texture.atlas_size(8) == (8, 16) and texture.atlas_size(9) == (16, 16)
    assert texture.atlas_size(2 ** 21) == (4096, 8192) and texture.atlas_size(2 ** 21 + 1) == (8192, 8192)      # 2048^2 = 2^22 units


def test_max_size_error_names_the_total_and_the_way_out():
    assert texture.atlas_size(64, 32) == (32, 32)
    with pytest.raises(ValueError, match=r"65 units.*--texture_scale.*simplify"):
        texture.atlas_size(65, 32)
    with pytest.raises(ValueError):
        texture.atlas_size(0)


# ---------------------------------------------------------------------------------------------------------------- the view
def test_view_rule_on_hand_made_votes():
    votes = np.array([[5, 0, 2, 0, 7, 1],
                      [5, 0, 3, 0, 7, 0],
                      [4, 0, 3, 9, 7, 0]])
    assert T.best_view(votes).tolist() == [0, -1, 1, 2, 0, 0]             # ties go to the lower view; no votes: unseen
    assert T.best_view(votes, min_px=3).tolist() == [0, -1, 1, 2, 0, -1]
    assert T.best_view(votes, min_px=8).tolist() == [-1, -1, -1, 2, -1, -1]
    assert T.best_view(votes[::-1]).tolist() == [1, -1, 0, 0, 0, 2]
    assert T.best_view(votes[:0]).tolist() == [-1] * 6
    # chunks: a running maximum over any split of the views
    big = np.random.RandomState(0).randint(0, 4, (9, 50))
    assert np.array_equal(T.best_view(big), T.best_view(np.concatenate([big[:8], big[8:]])))
    first = np.array([np.flatnonzero(col == col.max())[0] if col.max() > 0 else -1 for col in big.T])
    assert np.array_equal(T.best_view(big), first)


def test_restatement_cases_hold_what_the_gpu_tests_rely_on():
    """The plane looks away from view_cameras() as render_ref winds it and at them when reversed; the sphere has tied votes; the
    clutter mesh has the clamp at max_cell and the class of 4 in one atlas."""
    v, c, f, images, cams = T.case("unseen", 3)
    maps = R.render(v, f, cams, R.H, R.W)
    assert int(T.count_votes(maps["face"], maps["valid"], len(f)).sum()) == 0
    assert (T.reference("unseen", 3)["view"] == -1).all() and (T.reference("unseen", 3)["cell"][:, 2] == 4).all()
    assert (T.reference("plane", 3)["view"] >= 0).all()
    seen = {n: int((T.reference("sphere", n)["view"] >= 0).sum()) for n in (1, 3, 9)}
    print("sphere faces seen:", seen)
    assert seen == {1: 263, 3: 312, 9: 435}
    v, c, f, images, cams = T.case("sphere", 3)
    maps = R.render(v, f, cams, R.H, R.W)
    votes = T.count_votes(maps["face"], maps["valid"], len(f))
    tied = int(((votes == votes.max(0)).sum(0) > 1)[votes.max(0) > 0].sum())
    print("sphere faces with tied votes at 3 views:", tied)
    assert tied == 66
    cl = T.reference("clutter", 1, max_cell=64)
    assert cl["cell"][0, 2] == 64 and cl["view"][1] == -1 and set(np.unique(cl["cell"][2:, 2]).tolist()) == {4}
    wild = T.reference("wild", 3)
    assert (wild["view"] == -1).any() and (wild["view"] >= 0).any()


# ------------------------------------------------------------------------------------------------------------------- files
def test_obj_round_trip(tmp_path):
    ref = T.reference("sphere", 3)
    v, c, f, images, cams = T.case("sphere", 3)
    v = v.copy()
    v[0] = (np.float32(1.0) + np.float32(2.0 ** -23), np.float32(-3.4028235e38), np.float32(1e-45))     # awkward bits
    prefix = str(tmp_path / "ball_textured")
    texture.write_textured_obj(prefix, {"vertices": torch.from_numpy(v), "faces": torch.from_numpy(f)},
                               {k: torch.from_numpy(a) for k, a in ref.items()})
    got = texture.read_textured_obj(prefix + ".obj")
    assert got["mtllib"] == "ball_textured.mtl" and got["usemtl"] == "ball_textured"
    assert got["vertices"].dtype == np.float32 and np.array_equal(got["vertices"].view(np.uint32), v.view(np.uint32))
    assert np.array_equal(got["faces"], f)
    assert np.array_equal(got["face_vt"], np.arange(3 * len(f)).reshape(-1, 3))
    H, W = ref["atlas"].shape[:2]
    want = np.stack([ref["uv"][..., 0].reshape(-1) / W, 1.0 - ref["uv"][..., 1].reshape(-1) / H], 1)
    assert np.array_equal(got["vt"], want)                           # exact: W and H are powers of two
    assert np.array_equal(got["vt"][:, 0] * W, ref["uv"][..., 0].reshape(-1)) and np.array_equal((1.0 - got["vt"][:, 1]) * H, ref["uv"][..., 1].reshape(-1))
    assert got["atlas"].dtype == np.uint8 and np.array_equal(got["atlas"], ref["atlas"])
    # every vt lies inside its face's cell
    x, y = got["vt"][:, 0].reshape(-1, 3) * W, (1.0 - got["vt"][:, 1].reshape(-1, 3)) * H
    cell = ref["cell"]
    assert ((x >= cell[:, :1]) & (x <= cell[:, :1] + cell[:, 2:]) & (y >= cell[:, 1:2]) & (y <= cell[:, 1:2] + cell[:, 2:])).all()
    with pytest.raises(ValueError, match="atlas"):
        texture.write_textured_obj(prefix, {"vertices": v, "faces": f}, dict(ref, atlas=np.zeros((0, 0, 3), np.uint8)))
    with pytest.raises(ValueError, match="uv"):
        texture.write_textured_obj(prefix, {"vertices": v, "faces": f}, dict(ref, uv=ref["uv"][:-1]))


# ------------------------------------------------------------------------------------------------------------ command lines
BASE = ["--testpath", "a", "--testlist", "b", "--outdir", "c"]


@pytest.mark.parametrize("argv,word", [
    (["--texture"], "--mesh_voxel"),
    (["--fuse", "--texture"], "--mesh_voxel"),
    (["--fuse", "--mesh_voxel", "2", "--texture_scale", "2"], "belong to --texture"),
    (["--fuse", "--mesh_voxel", "2", "--texture_min_px", "3"], "belong to --texture"),
    (["--fuse", "--mesh_voxel", "2", "--texture", "--texture_scale", "0"], "scale"),
    (["--fuse", "--mesh_voxel", "2", "--texture", "--texture_scale", "nan"], "scale"),
    (["--fuse", "--mesh_voxel", "2", "--texture", "--texture_max_cell", "48"], "max_cell"),
    (["--fuse", "--mesh_voxel", "2", "--texture", "--texture_max_size", "100000"], "max_size"),
    (["--fuse", "--mesh_voxel", "2", "--texture", "--texture_min_px", "0"], "min_px"),
])
def test_infer_refuses_texture_options_that_do_not_fit(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        infer.parse_args(BASE + argv)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_infer_accepts_texture_options():
    args = infer.parse_args(BASE + ["--fuse", "--mesh_voxel", "2", "--texture", "--texture_scale", "0.5", "--texture_max_cell", "64"])
    assert args.texture and args.texture_kw == dict(scale=0.5, max_cell=64, max_size=16384, min_px=1)
    args = infer.parse_args(BASE + ["--fuse", "--mesh_voxel", "2"])
    assert not args.texture and args.texture_kw == {}


@pytest.mark.parametrize("argv,word", [(["--texture_scale", "-1"], "scale"), (["--texture_max_cell", "2"], "max_cell"),
                                       (["--texture_max_size", "3"], "max_size"), (["--texture_min_px", "-4"], "min_px")])
def test_texture_command_line_refuses_values_outside_their_range(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        texture.main(BASE + argv)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_library_call_checks_its_arguments_before_the_device():
    """Shapes, dtypes and ranges are ValueErrors; a CPU tensor is a RuntimeError.  Nothing is launched: there is no GPU here."""
    v, c, f, images, cams = T.case("plane", 2)
    mesh = {"vertices": torch.from_numpy(v), "colors": torch.from_numpy(c), "faces": torch.from_numpy(f)}
    ti, tc = torch.from_numpy(images), torch.from_numpy(cams)
    for bad in (dict(images=ti.float()), dict(images=ti[..., :2]), dict(images=ti[0]), dict(cams=tc[:1]), dict(cams=tc[:, 0]),
                dict(scale=0.0), dict(scale=float("inf")), dict(max_cell=24), dict(max_cell=8192), dict(max_size=2), dict(min_px=0),
                dict(chunk=0), dict(chunk=33)):
        kw = dict(images=ti, cams=tc)
        kw.update(bad)
        with pytest.raises(ValueError):
            texture.texture_mesh(mesh, **kw)
    for key, t in (("vertices", mesh["vertices"].double()), ("faces", mesh["faces"].long()), ("colors", mesh["colors"][:-1])):
        with pytest.raises(ValueError):
            texture.texture_mesh(dict(mesh, **{key: t}), ti, tc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        texture.texture_mesh(mesh, ti, tc)


# ------------------------------------------------------------------------------------------------------------------ quality
def test_texture_is_closer_to_the_surface_colour_than_vertex_colours():
    """A coarse plane of 8 faces that look at three cameras, carrying an analytic pattern of several periods per face.  Each view's
    image is the pattern at every pixel centre's ray-plane intersection.  The atlas of the restatement, read back at the UVs of
    a dense set of surface points, against the colours interpolated from the 9 vertices: rms error over the channels.
    Measured: 0.85 for the atlas against 80.68 for the vertex colours (levels of 255)."""
    v, f = R.plane_mesh(3)
    f = T.reversed_faces(f)
    assert len(f) == 8
    cams = R.view_cameras(3)
    h, w = 96, 128
    cams = cams.copy()
    cams[:, 1, :2, :3] *= 2.0                                        # the cameras of render_ref at twice the resolution
    images = T.plane_images(cams, h, w)
    vc = np.floor(np.clip(T.pattern(v.astype(np.float64)), 0, 255) + 0.5).astype(np.uint8)
    out = T.texture(v, vc, f, images, cams)
    assert (out["view"] >= 0).all()
    # dense surface points: barycentric lattice centroids of every face
    n = 24
    pts, uvs, flat = [], [], []
    V64 = v.astype(np.float64)
    for k, (a, b, c) in enumerate(f):
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        keep = i + j < n - 1
        wb, wc = (i[keep] + 0.33) / n, (j[keep] + 0.33) / n
        wa = 1.0 - wb - wc
        pts.append(wa[:, None] * V64[a] + wb[:, None] * V64[b] + wc[:, None] * V64[c])
        uv = out["uv"][k].astype(np.float64)
        uvs.append(wa[:, None] * uv[0] + wb[:, None] * uv[1] + wc[:, None] * uv[2])
        flat.append(wa[:, None] * vc[a].astype(np.float64) + wb[:, None] * vc[b] + wc[:, None] * vc[c])
    pts, uvs, flat = np.concatenate(pts), np.concatenate(uvs), np.concatenate(flat)
    truth = T.pattern(pts)
    rms_atlas = float(np.sqrt(((T.atlas_lookup(out["atlas"], uvs) - truth) ** 2).mean()))
    rms_vertex = float(np.sqrt(((flat - truth) ** 2).mean()))
    print(f"rms error against the pattern over {len(pts)} surface points: atlas {rms_atlas:.2f}, vertex colours {rms_vertex:.2f}")
    assert rms_atlas < rms_vertex
