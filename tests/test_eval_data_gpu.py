"""cds_mvsnet_amd.eval_data on the GPU: ops.eval_views bit for bit against the numpy restatement (tests/eval_data_ref.py) and within
its rounding bound of float64, ops.eval_outputs bit for bit against the host arithmetic of mvs_io.save_outputs, EvalViews samples
against EvalScenes and the reference-written G10 fixtures, the view cache, and infer --pipeline gpu against --pipeline host file by
file."""
import os
import threading

import numpy as np
import pytest
import torch

import eval_data_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- ops.eval_views ----------------------------------------------------------------------------------------------------------------
def _views(V, Hs, Ws, pad, h, w):
    from cds_mvsnet_amd import eval_data as E
    from cds_mvsnet_amd import ops
    src = R.random_u8((V, Hs, Ws, 3), seed=Hs + Ws + V)
    junk = [torch.empty(k, device=DEV) for k in (3, 1001, 77)]          # a used allocator
    del junk[1]
    rows, cols = E.view_tables(Hs, Ws, pad, h, w, DEV)
    got = ops.eval_views(torch.from_numpy(src).to(DEV), rows, cols)
    assert got.dtype == torch.float32 and tuple(got.shape) == (V, 3, h, w) and got.is_contiguous()
    return src, got.cpu()


@pytest.mark.parametrize("V,src,pad,dst", [(3, (37, 53), 0, (32, 48)),          # shrink, non-integer ratio
                                           (2, (16, 24), 0, (32, 48)),          # enlarge: both clamps
                                           (2, (50, 70), 0, (30, 45)),          # w % 4 != 0: the scalar tail
                                           (1, (100, 160), 4, (54, 80)),        # padding and resize together
                                           (5, (70, 90), 0, (64, 96))])         # several workgroups, one axis down and one up
def test_eval_views_equals_the_restatement(V, src, pad, dst):
    u8, got = _views(V, src[0], src[1], pad, dst[0], dst[1])
    worst = 0.0
    for i in range(V):
        assert torch.equal(got[i], torch.from_numpy(R.resize(u8[i], dst[0], dst[1], pad, np.float32))), i
        f64 = R.resize(u8[i], dst[0], dst[1], pad, np.float64)
        worst = max(worst, float(np.abs(got[i].numpy().astype(np.float64) - f64).max()))
    print(f"max |gpu - f64| = {worst / 2 ** -24:.3f} * 2^-24")
    assert worst <= 2.0 ** -22                                 # six roundings of at most 2^-25 on values <= 1 (test_eval_data_cpu.py)


def test_eval_views_padding_without_resize_is_exact():
    u8, got = _views(1, 24, 40, 4, 32, 40)
    want = np.pad(np.array(u8[0], dtype=np.float32) / 255., ((4, 4), (0, 0), (0, 0)), "edge").transpose(2, 0, 1)
    assert torch.equal(got[0], torch.from_numpy(np.ascontiguousarray(want)))
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)
    from cds_mvsnet_amd import eval_data as E
    from cds_mvsnet_amd import ops
    got = ops.eval_views(torch.from_numpy(u8).to(DEV), *E.view_tables(16, 16, 0, 16, 16, DEV)).cpu()       # no padding either: u8 / 255
    assert torch.equal(got[0, 1], torch.from_numpy(np.arange(256, dtype=np.float32).reshape(16, 16) / 255.))


def test_eval_views_errors():
    from cds_mvsnet_amd import eval_data as E
    from cds_mvsnet_amd import ops
    src = torch.zeros(2, 8, 12, 3, dtype=torch.uint8, device=DEV)
    rows, cols = E.view_tables(8, 12, 0, 8, 12, DEV)
    assert ops.eval_views(src, rows, cols).shape == (2, 3, 8, 12)
    other = E.view_tables(8, 12, 0, 6, 12, DEV)[0]             # 6 entries
    bad = [(src.float(), rows, cols),                          # wrong dtype
           (src[0], rows, cols), (src[..., :2], rows, cols),   # wrong rank / not 3 channels
           (src.cpu(), rows, cols),                            # host tensor
           (src.transpose(1, 2), rows, cols),                  # not contiguous
           (src, (rows[0], other[1], rows[2]), cols),          # mismatched table lengths
           (src, rows, (cols[0], cols[1], cols[2][:-1])),
           (src, (rows[0], rows[1], rows[2].double()), cols),  # weights not float32
           (src, (rows[0].long(), rows[1], rows[2]), cols),    # taps not int32
           (src, tuple(t.cpu() for t in rows), cols),          # tables on the host
           (src, rows[:2], cols)]
    for args in bad:
        with pytest.raises(ValueError):
            ops.eval_views(*args)


# ---- ops.eval_outputs --------------------------------------------------------------------------------------------------------------
def _image(H, W, seed):
    """[3,H,W] in [0,1] with the awkward values: k / 255 for every k (1.0 * 255 is exactly 255.0), the float32 just below each, and
    values outside [0,1] for the clip."""
    rs = np.random.RandomState(seed)
    img = rs.rand(3, H, W).astype(np.float32)
    flat = img.reshape(-1)
    ks = np.arange(256, dtype=np.float32) / np.float32(255)
    flat[:256] = ks
    flat[256:512] = np.nextafter(ks, np.float32(-1))
    flat[512:520] = [1.0, 1.0000001, 1.5, -0.25, -0.0, 0.99999994, 0.003921569, 254.99999 / 255]
    return img


@pytest.mark.parametrize("shapes,dst", [(((16, 24), (32, 48), (64, 96)), (64, 96)),          # no refinement
                                        (((16, 24), (32, 48), (64, 96)), (128, 192)),        # refinement: every map is upsampled
                                        (((40, 56), (80, 112), (160, 224)), (150, 210)),     # non-integer ratio, w % 4 != 0
                                        (((5, 7), (10, 14), (20, 28)), (20, 28))])
def test_eval_outputs_equals_save_outputs_arithmetic(shapes, dst):
    from cds_mvsnet_amd import eval_data as E
    from cds_mvsnet_amd import mvs_io, ops
    rs = np.random.RandomState(sum(dst))
    confs = [rs.rand(*s).astype(np.float32) for s in shapes]
    img = _image(shapes[2][0], shapes[2][1], seed=dst[0]) if shapes[2][0] * shapes[2][1] * 3 >= 520 else rs.rand(3, *shapes[2]).astype(np.float32)
    h, w = dst
    tab = E.output_tables(list(shapes) + [img.shape[1:]], h, w, DEV)
    conf3, img_u8 = ops.eval_outputs([torch.from_numpy(c).to(DEV) for c in confs], torch.from_numpy(img).to(DEV), tab, h, w)
    want_conf, want_img = R.outputs(confs, img, h, w)
    assert np.array_equal(want_conf[..., 0], mvs_io.nearest_resize(confs[0], h, w))         # the restatement is nearest_resize
    assert conf3.dtype == torch.float32 and img_u8.dtype == torch.uint8 and tuple(conf3.shape) == tuple(img_u8.shape) == (h, w, 3)
    assert torch.equal(conf3.cpu(), torch.from_numpy(want_conf))
    assert torch.equal(img_u8.cpu(), torch.from_numpy(want_img))
    if img.size >= 520 and dst == shapes[2]:
        assert want_img.max() == 255 and want_img.min() == 0 and len(np.unique(want_img)) == 256


def test_eval_outputs_errors():
    from cds_mvsnet_amd import eval_data as E
    from cds_mvsnet_amd import ops
    confs = [torch.rand(4, 6, device=DEV), torch.rand(8, 12, device=DEV), torch.rand(16, 24, device=DEV)]
    img = torch.rand(3, 16, 24, device=DEV)
    tab = E.output_tables([(4, 6), (8, 12), (16, 24), (16, 24)], 16, 24, DEV)
    assert ops.eval_outputs(confs, img, tab, 16, 24)[0].shape == (16, 24, 3)
    bad = [(confs[:2], img, tab, 16, 24),
           ([confs[0].double()] + confs[1:], img, tab, 16, 24),
           ([confs[0].cpu()] + confs[1:], img, tab, 16, 24),
           ([confs[0].t()] + confs[1:], img, tab, 16, 24),
           (confs, img[:2], tab, 16, 24), (confs, img.cpu(), tab, 16, 24), (confs, img.transpose(1, 2), tab, 16, 24),
           (confs, img, tab[:-1], 16, 24), (confs, img, tab, 16, 20), (confs, img, tab.long(), 16, 24), (confs, img, tab.cpu(), 16, 24)]
    for args in bad:
        with pytest.raises(ValueError):
            ops.eval_outputs(*args)


# ---- EvalViews against EvalScenes --------------------------------------------------------------------------------------------------
def _assert_sample_equal(got, want, imgs=True):
    assert got["imgs"].is_cuda and got["imgs"].dtype == torch.float32 and got["imgs"].shape[0] == 1
    if imgs:
        assert torch.equal(got["imgs"][0].cpu(), torch.from_numpy(want["imgs"]))
    assert got["filename"] == want["filename"]
    assert got["depth_values"].dtype == want["depth_values"].dtype and np.array_equal(got["depth_values"], want["depth_values"])
    assert sorted(got["proj_matrices"]) == sorted(want["proj_matrices"])
    for k, m in want["proj_matrices"].items():
        assert got["proj_matrices"][k].dtype == m.dtype and np.array_equal(got["proj_matrices"][k], m), k


@pytest.mark.parametrize("refine", [False, True])
def test_samples_equal_eval_scenes_synthetic(tmp_path, refine):
    from cds_mvsnet_amd import mvs_io
    from cds_mvsnet_amd.eval_data import EvalViews
    R.write_scene(str(tmp_path), "scan1", 4, 64, 96, seed=1)
    kw = dict(nviews=3, ndepths=192, interval_scale=1.06, max_h=64, max_w=96, refine=refine)
    host = mvs_io.EvalScenes(str(tmp_path), ["scan1"], **kw)
    start = threading.active_count()
    with EvalViews(str(tmp_path), ["scan1"], device=DEV, **kw) as it:
        assert len(it) == len(host) == 4
        got = list(it)
    assert threading.active_count() == start and len(got) == 4
    for idx, g in enumerate(got):
        assert tuple(g["imgs"].shape) == (1, 3, 3, 64, 96)
        _assert_sample_equal(g, host[idx])
    assert it.stats["decodes"] == 4 and it.stats["evictions"] == 0 and it.stats["hits"] == 8       # 12 views served, 4 decoded


@pytest.mark.parametrize("dataset", ["dtu", "tt"])
@pytest.mark.parametrize("refine", [False, True])
def test_samples_equal_eval_scenes_and_the_reference_fixture(tmp_path, golden, dataset, refine):
    """The G10 scenes (tests/test_mvs_io.py): EvalViews == EvalScenes on every sample, and its images == the arrays the REFERENCE's
    dataset wrote (the tt layout pads 56 -> 64 rows and moves the principal point)."""
    from cds_mvsnet_amd import mvs_io
    from cds_mvsnet_amd.eval_data import EvalViews
    g = golden("g10_formats")
    for i, name in enumerate(g["scene_file_names"]):
        p = tmp_path / str(name)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(g[f"scene_file_{i}"].tobytes())
    scan = "scan_" + dataset
    kw = dict(nviews=4, ndepths=192, interval_scale=1.06, max_h=64, max_w=80, refine=refine, dataset=dataset)
    host = mvs_io.EvalScenes(str(tmp_path / dataset), [scan], **kw)
    with EvalViews(str(tmp_path / dataset), [scan], device=DEV, ahead=0, **kw) as it:
        got = list(it)
    assert len(got) == len(host) == 4
    for idx, smp in enumerate(got):
        _assert_sample_equal(smp, host[idx])
        if idx in (0, 2):
            key = f"scene_{dataset}_{'refine' if refine else 'norefine'}_{idx}"
            assert torch.equal(smp["imgs"][0].cpu(), g[key + "_imgs"])
            assert smp["filename"] == str(g[key + "_filename"])


def test_resized_views_follow_the_linear_rule(tmp_path):
    """100 x 140 JPEGs into 64 x 96: the images are the restatement applied to the bytes PIL decodes (NOT EvalScenes's PIL resize);
    cameras, depth values and names are EvalScenes's."""
    from cds_mvsnet_amd import mvs_io
    from cds_mvsnet_amd.eval_data import EvalViews
    R.write_scene(str(tmp_path), "s", 4, 100, 140, seed=2)
    kw = dict(nviews=3, max_h=64, max_w=96)
    host = mvs_io.EvalScenes(str(tmp_path), ["s"], **kw)
    with EvalViews(str(tmp_path), ["s"], device=DEV, **kw) as it:
        got = list(it)
    differs = 0
    for idx, g in enumerate(got):
        want = host[idx]
        _assert_sample_equal(g, want, imgs=False)
        _, ref, srcs = host.metas[idx]
        for n, vid in enumerate([ref] + srcs):
            assert torch.equal(g["imgs"][0, n].cpu(), torch.from_numpy(R.resize(R.decoded(str(tmp_path), "s", vid), 64, 96))), (idx, vid)
        differs += int(not np.array_equal(g["imgs"][0].cpu().numpy(), want["imgs"]))
    assert differs == 4                                        # random pixels: the antialiasing PIL filter gives other values
    # the same through the Tanks & Temples padding: 100 + 8 rows resized to 64
    with EvalViews(str(tmp_path), ["s"], device=DEV, dataset="tt", **kw) as it:
        g = next(it)
    want = mvs_io.EvalScenes(str(tmp_path), ["s"], dataset="tt", **kw)[0]
    _assert_sample_equal(g, want, imgs=False)
    assert torch.equal(g["imgs"][0, 1].cpu(), torch.from_numpy(R.resize(R.decoded(str(tmp_path), "s", 1), 64, 96, pad=4)))


def test_small_cache_evicts_and_samples_do_not_change(tmp_path):
    from cds_mvsnet_amd.eval_data import EvalViews
    R.write_scene(str(tmp_path), "s", 4, 64, 96, seed=3)
    kw = dict(nviews=3, max_h=64, max_w=96, device=DEV)
    with EvalViews(str(tmp_path), ["s"], **kw) as it:
        want = [s["imgs"].cpu() for s in it]
    two_views = 2 * 3 * 64 * 96 * 4 / 2 ** 20
    for ahead in (0, 2):
        with EvalViews(str(tmp_path), ["s"], cache_mb=two_views, ahead=ahead, **kw) as it:
            got = [s["imgs"].cpu() for s in it]
        assert it.stats["evictions"] > 0 and it.stats["decodes"] > 4 and len(it.cache) <= 2
        assert it.stats["decodes"] + it.stats["hits"] == 12
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))
    with EvalViews(str(tmp_path), ["s"], cache_mb=0, **kw) as it:               # below one view: served, never kept
        got = [s["imgs"].cpu() for s in it]
    assert len(it.cache) == 0 and all(torch.equal(a, b) for a, b in zip(got, want))
    # a subset of the metas in another order, as a rank of several takes them
    with EvalViews(str(tmp_path), ["s"], indices=[3, 1], **kw) as it:
        got = [s["imgs"].cpu() for s in it]
    assert len(got) == 2 and torch.equal(got[0], want[3]) and torch.equal(got[1], want[1])
    with EvalViews(str(tmp_path), ["s"], rank=1, world=2, **kw) as it:          # infer's sharding: idx % world == rank
        got = [s["imgs"].cpu() for s in it]
    assert it.order == [1, 3] and len(got) == 2 and torch.equal(got[0], want[1]) and torch.equal(got[1], want[3])
    with pytest.raises(ValueError):
        EvalViews(str(tmp_path), ["s"], rank=2, world=2, **kw)
    torch.cuda.synchronize()


def test_worker_error_is_reraised(tmp_path):
    from cds_mvsnet_amd.eval_data import EvalViews
    R.write_scene(str(tmp_path), "s", 4, 64, 96, seed=4)
    bad = os.path.join(str(tmp_path), "s", "images", "00000003.jpg")
    with open(bad, "r+b") as f:                                # the header survives (its size is read when the sample is scheduled)
        f.truncate(os.path.getsize(bad) // 2)
    start = threading.active_count()
    it = EvalViews(str(tmp_path), ["s"], nviews=3, max_h=64, max_w=96, device=DEV)
    with pytest.raises(OSError):                               # view 3 is the reference view of the last sample only
        for _ in range(4):
            next(it)
    assert threading.active_count() == start
    torch.cuda.synchronize()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(d, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_infer_gpu_pipeline_writes_the_same_bytes_as_host(tmp_path):
    from cds_mvsnet_amd import infer
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    R.write_scene(root, "scanA", 4, 128, 160, seed=5)
    with open(tmp_path / "list.txt", "w") as f:
        f.write("scanA\n")
    trees = {}
    start = threading.active_count()
    for pipeline in ("host", "gpu"):
        out = str(tmp_path / pipeline)
        infer.main(["--testpath", root, "--testlist", str(tmp_path / "list.txt"), "--outdir", out, "--num_view", "3", "--max_h", "128",
                    "--max_w", "160", "--interval_scale", "1.0", "--save_stages", "--fuse", "--thres_view", "1", "--pipeline", pipeline])
        trees[pipeline] = _tree(out)
    assert threading.active_count() == start
    names = sorted(trees["host"])
    assert names == sorted(trees["gpu"])
    for sub, ext in (("depth_est", ".pfm"), ("confidence", ".pfm"), ("cams", "_cam.txt"), ("images", ".jpg"), ("depth_stage1", ".pfm"),
                     ("depth_stage2", ".pfm"), ("depth_stage3", ".pfm")):
        for v in range(4):
            assert os.path.join("scanA", sub, f"{v:08d}{ext}") in names
    assert "scanA.ply" in names and len(names) == 4 * 7 + 1
    for n in names:
        assert trees["host"][n] == trees["gpu"][n], n
