"""cds_mvsnet_amd.train_data / fit, the host side: metas, cameras, depth values, view choice, the epoch's order, checkpoints and fast
failure, against tests/train_data_ref.py.  Everything here runs without a GPU (dataset.load is host-only)."""
import os

import numpy as np
import pytest
import torch

import train_data_ref as TR
from cds_mvsnet_amd import train_data as TD

BLENDED_PAIRS = [(0, [1, 2, 3, 4, 5, 6, 7, 8, 9]),            # more than 7 sources: train mode uses the first 7 only
                 (1, []),                                      # no source view: dropped
                 (2, [0, 3]),                                  # 2 sources at nviews = 5: padded with src_views[0]
                 (3, [0, 1, 2, 4, 5])]
BLENDED_LINES = ["425.0 2.5 128 745.0", "425.0 2.5", "430.5 1.75 100.0 900.0", "425.0 2.5 128 745.0"] + ["425.0 2.5 128 745.0"] * 6


@pytest.fixture(scope="module")
def dtu(tmp_path_factory):
    root = tmp_path_factory.mktemp("dtu")
    lst = TR.write_dtu_tree(root, scans=("scan1", "scan9"), n_views=3, image_hw=(16, 24), gt_hw=(38, 54), seed=3)
    return str(root), lst


@pytest.fixture(scope="module")
def blended(tmp_path_factory):
    root = tmp_path_factory.mktemp("blended")
    lst = TR.write_blended_tree(root, scans=("sceneA", "sceneB"), n_views=10, pairs=BLENDED_PAIRS, image_hw=(20, 28), seed=4,
                                depth_lines=BLENDED_LINES)
    return str(root), lst


def _plain(metas):
    return [tuple(list(x) if isinstance(x, (tuple, list)) else x for x in m) for m in metas]


def test_dtu_metas(dtu):
    root, lst = dtu
    ds = TD.DTUTrainScenes(root, lst, "train", 3, crop=(16, 24))
    assert len(ds) == 2 * 3 * 7
    assert _plain(ds.metas) == _plain(TR.dtu_metas(root, lst))
    assert [m[:3] for m in ds.metas[:8]] == [("scan1", l, 0) for l in range(7)] + [("scan1", 0, 1)]   # scan x viewpoint x light
    assert ds.metas[-1][:3] == ("scan9", 6, 2)


def test_blended_metas(blended):
    root, lst = blended
    ds = TD.BlendedTrainScenes(root, lst, "train", 5, crop=(16, 24))
    assert _plain(ds.metas) == _plain(TR.blended_metas(root, lst, 5))
    assert len(ds) == 2 * 3 and [m[1] for m in ds.metas[:3]] == [0, 2, 3]             # viewpoint 1 has no source: dropped
    assert list(ds.metas[1][2]) == [0, 3, 0, 0, 0]                                     # padded with src_views[0] up to nviews
    assert list(TD.BlendedTrainScenes(root, lst, "train", 3, crop=(16, 24)).metas[1][2]) == [0, 3, 0]


@pytest.mark.parametrize("layout", ["dtu", "blended"])
def test_load_matches_the_restatement(layout, dtu, blended):
    root, lst = dtu if layout == "dtu" else blended
    crop, nviews, ndepths, scale = (16, 24), 3, 48, 1.06
    cls = TD.DTUTrainScenes if layout == "dtu" else TD.BlendedTrainScenes
    ds = cls(root, lst, "val", nviews, ndepths=ndepths, interval_scale=scale, crop=crop)
    metas = TR.dtu_metas(root, lst) if layout == "dtu" else TR.blended_metas(root, lst, nviews)
    for index in range(len(ds)):
        got = ds.load(index, 0)
        want = TR.sample(layout, root, metas, index, "val", nviews, ndepths, scale, crop)
        ms = TD.stage_matrices(got["proj"])
        for k in TR.STAGES:
            assert ms[k].dtype == np.float32 and np.array_equal(ms[k], want["proj_matrices"][k]), (index, k)
        assert np.array_equal(ms["stage1"][:, 1, :2], ms["stage2"][:, 1, :2] * np.float32(0.5))
        assert np.array_equal(ms["stage4"][:, 1, :2], ms["stage2"][:, 1, :2] * np.float32(4))
        assert np.array_equal(ms["stage4"][:, 0], got["proj"][:, 0]) and np.array_equal(ms["stage3"][:, 1, 2], got["proj"][:, 1, 2])
        assert got["depth_values"].dtype == np.float32 and np.array_equal(got["depth_values"], want["depth_values"])
        assert got["filename"] == want["filename"]
        assert got["imgs"].dtype == np.uint8 and got["imgs"].shape[0] == nviews and got["imgs"].shape[3] == 3
        assert (got["mask8"] is not None) == (layout == "dtu")


def test_blended_cameras(blended):
    root, lst = blended
    ds = TD.BlendedTrainScenes(root, lst, "val", 3, ndepths=48, interval_scale=1.06, crop=(16, 24))
    from cds_mvsnet_amd import mvs_io
    raw = mvs_io.read_cam_file(os.path.join(root, "sceneA/cams/00000002_cam.txt"))[0]
    intr, _, dmin, interval = ds._read_cam(os.path.join(root, "sceneA/cams/00000002_cam.txt"))
    assert np.array_equal(intr[:2], raw[:2] / np.float32(4.0)) and np.array_equal(intr[2], raw[2])     # the principal point only scales
    # three (or more) values on line 11: the range is re-spread over ndepths planes, then scaled
    assert dmin == 430.5 and interval == ((430.5 + int(float("100.0")) * 1.75) - 430.5) / 48 * 1.06
    # two values: the interval as written, scaled
    _, _, dmin1, interval1 = ds._read_cam(os.path.join(root, "sceneA/cams/00000001_cam.txt"))
    assert dmin1 == 425.0 and interval1 == 2.5 * 1.06
    dv = ds.load(1, 0)["depth_values"]                        # meta 1 = viewpoint 2
    assert np.array_equal(dv, np.arange(430.5, interval * (48 - 0.5) + 430.5, interval, dtype=np.float32)) and len(dv) == 48


def test_dtu_depth_values_length(dtu):
    root, lst = dtu
    for ndepths, n in ((192, 192), (48, 49)):                 # float arithmetic: 425 + 48 * 2.65 lands past the last plane
        ds = TD.DTUTrainScenes(root, lst, "val", 3, ndepths=ndepths, interval_scale=1.06, crop=(16, 24))
        dv = ds.load(0, 0)["depth_values"]
        want = TR.depth_values("dtu", 425.0, 2.5 * 1.06, ndepths)
        assert len(dv) == n == len(want) and np.array_equal(dv, want)


def test_view_choice(dtu, blended):
    root, lst = blended
    val = TD.BlendedTrainScenes(root, lst, "val", 5, crop=(16, 24), seed=11)
    assert val.view_ids(0, 0) == [0, 1, 2, 3, 4] == val.view_ids(0, 3)
    a = TD.BlendedTrainScenes(root, lst, "train", 5, crop=(16, 24), seed=11)
    b = TD.BlendedTrainScenes(root, lst, "train", 5, crop=(16, 24), seed=11)
    metas = TR.blended_metas(root, lst, 5)
    before = _plain(a.metas)
    seen = set()
    for epoch in range(6):
        for index in range(len(a)):
            ids = a.view_ids(index, epoch)
            assert ids == b.view_ids(index, epoch) == TR.view_ids("blended", metas[index], "train", 5, 11, epoch, index)
            assert ids[0] == a.metas[index][1] and len(ids) == 5
            if index == 0:
                assert set(ids[1:]) <= set(range(1, 8)) and len(set(ids[1:])) == 4      # a permutation of the FIRST 7 sources
                seen.add(tuple(ids))
    assert len(seen) > 1                                       # the epoch matters
    assert a.view_ids(0, 0) != TD.BlendedTrainScenes(root, lst, "train", 5, crop=(16, 24), seed=12).view_ids(0, 0) or \
        a.view_ids(0, 1) != TD.BlendedTrainScenes(root, lst, "train", 5, crop=(16, 24), seed=12).view_ids(0, 1)
    a.load(0, 2), a.load(1, 2)
    assert _plain(a.metas) == before                           # the stored metas are never shuffled in place
    root, lst = dtu
    d = TD.DTUTrainScenes(root, lst, "train", 3, crop=(16, 24), seed=5)
    dm = TR.dtu_metas(root, lst)
    before = _plain(d.metas)
    for index in (0, 7, 20):
        ids = d.view_ids(index, 1)
        assert ids == TR.view_ids("dtu", dm[index], "train", 3, 5, 1, index) and sorted(ids) == [0, 1, 2]
        d.load(index, 1)
    assert _plain(d.metas) == before
    assert TD.DTUTrainScenes(root, lst, "val", 3, crop=(16, 24)).view_ids(7, 4) == [1, 0, 2]


def test_load_into_staging_arrays(dtu):
    root, lst = dtu
    ds = TD.DTUTrainScenes(root, lst, "train", 3, crop=(16, 24))
    assert ds.sizes() == ((16, 24), (38, 54))
    out = (np.zeros((3, 16, 24, 3), np.uint8), np.zeros((38, 54), np.float32), np.zeros((38, 54), np.uint8))
    a, b = ds.load(5, 1), ds.load(5, 1, out)
    assert b["imgs"] is out[0] and b["depth"] is out[1] and b["mask8"] is out[2]
    for k in ("imgs", "depth", "mask8", "proj", "depth_values"):
        assert np.array_equal(a[k], b[k]), k
    assert len(set(map(int, np.unique(a["mask8"])))) > 2
    with pytest.raises(ValueError, match="depth_map"):
        ds.load(5, 1, (out[0], np.zeros((40, 54), np.float32), out[2]))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sampler(world):
    n, B = 23, 2
    full = TD.epoch_batches(n, B, seed=3, epoch=4)
    assert len(full) == n // B and sorted(i for b in full for i in b) == sorted(set(i for b in full for i in b))
    shards = [TD.epoch_batches(n, B, seed=3, epoch=4, rank=r, world=world) for r in range(world)]
    assert len({len(s) for s in shards}) == 1 and len(shards[0]) == len(full) // world
    flat = [tuple(b) for s in shards for b in s]
    assert len(set(flat)) == len(flat)                                                   # disjoint
    keep = len(full) - len(full) % world
    assert sorted(flat) == sorted(tuple(b) for b in full[:keep])                          # the epoch's batches minus the trimmed tail
    for r in range(world):
        assert shards[r] == full[:keep][r::world]
        assert shards[r] == TD.epoch_batches(n, B, seed=3, epoch=4, rank=r, world=world)   # the same epoch: the same order
    assert TD.epoch_batches(n, B, seed=3, epoch=5) != full and TD.epoch_batches(n, B, seed=4, epoch=4) != full
    # no shuffle, keep the short batch (validation)
    plain = TD.epoch_batches(5, 2, shuffle=False, drop_last=False)
    assert plain == [[0, 1], [2, 3], [4]]
    with pytest.raises(ValueError):
        TD.epoch_batches(5, 2, rank=2, world=2)


def test_checkpoint_round_trip(tmp_path, seeded_state):
    from cds_mvsnet_amd import CDSMVSNet, fit, infer
    model = seeded_state(True)
    path = str(tmp_path / "checkpoint-epoch3.pth")
    fit.save_checkpoint(path, model, 3, float("inf"), {"arch": {"type": "CDSMVSNet", "args": {"refine": True}}, "lr": 1e-4})
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert tuple(ck) == ("arch", "epoch", "state_dict", "monitor_best", "config") == fit.CHECKPOINT_KEYS
    assert ck["arch"] == "CDSMVSNet" and ck["epoch"] == 3 and ck["monitor_best"] == float("inf")
    fresh = CDSMVSNet(refine=True, ndepths=(48, 32, 8), depth_interals_ratio=(4.0, 1.5, 0.75))
    infer.load_checkpoint(fresh, path)                         # no trust_pickle: the file holds tensors and builtins only
    want, got = model.state_dict(), fresh.state_dict()
    assert list(want) == list(got)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    with pytest.raises(TypeError):
        fit.save_checkpoint(path, model, 3, 0.0, {"parser": object()})
    assert fit.parse_monitor("off") == (None, None) and fit.parse_monitor("min abs_depth_error") == ("min", "abs_depth_error")
    with pytest.raises(ValueError):
        fit.parse_monitor("smallest loss")


def test_a_missing_image_fails_fast_with_its_path(tmp_path):
    lst = TR.write_blended_tree(tmp_path, n_views=4, image_hw=(20, 28), seed=6)
    ds = TD.BlendedTrainScenes(str(tmp_path), lst, "val", 3, crop=(16, 24))
    gone = os.path.join(str(tmp_path), "sceneA/blended_images/00000002.jpg")
    os.remove(gone)
    it = TD.TrainBatches(ds, 2, "cuda", epoch=0, ahead=0)     # the check runs before any device call: no GPU needed to get here
    with pytest.raises(FileNotFoundError) as e:
        next(iter(it))
    assert gone in str(e.value)
    with pytest.raises(StopIteration):                        # the iterator is closed
        next(it)


def test_a_grayscale_image_raises(tmp_path):
    from PIL import Image
    lst = TR.write_blended_tree(tmp_path, n_views=4, image_hw=(20, 28), seed=6)
    ds = TD.BlendedTrainScenes(str(tmp_path), lst, "val", 3, crop=(16, 24))
    bad = os.path.join(str(tmp_path), "sceneA/blended_images/00000001.jpg")
    Image.fromarray(np.full((20, 28), 128, np.uint8)).save(bad)
    with pytest.raises(ValueError) as e:
        ds.load(0, 0)
    assert bad in str(e.value)


def test_arguments():
    with pytest.raises(ValueError):
        TD.epoch_batches(4, 0)
    from cds_mvsnet_amd import fit
    args = fit.parse_args(["--dataset", "dtu", "--datapath", "a", "--trainlist", "b", "--vallist", "c", "--dataset", "blended",
                           "--datapath", "d", "--trainlist", "e", "--vallist", "f", "--monitor", "min abs_depth_error", "--graph"])
    assert args.dataset == ["dtu", "blended"] and args.dlossw == [0.5, 1.0, 2.0] and args.graph and args.threads == 4 and args.ahead == 2
    with pytest.raises(SystemExit):
        fit.parse_args(["--dataset", "dtu", "--datapath", "a", "--trainlist", "b", "--dataset", "blended"])
