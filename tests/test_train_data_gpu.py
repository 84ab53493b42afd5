"""cds_mvsnet_amd.train_data / fit on the GPU: ops.image_batch bit for bit against numpy, a batch of both layouts bit for bit against
tests/train_data_ref.py, decode-ahead against the synchronous path, shutdown, and fit end to end."""
import math
import os
import threading

import numpy as np
import pytest
import torch

import train_data_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- ops.image_batch --------------------------------------------------------------------------------------------------------------
def _source(n, Hs, Ws, seed):
    """uint8 [n,Hs,Ws,3]; with 256 pixels or more every channel of every image holds all 256 byte values."""
    rs = np.random.RandomState(seed)
    src = rs.randint(0, 256, (n, Hs * Ws, 3)).astype(np.uint8)
    if Hs * Ws >= 256:
        for i in range(n):
            for c in range(3):
                src[i, rs.permutation(Hs * Ws)[:256], c] = rs.permutation(256)
                assert len(np.unique(src[i, :, c])) == 256
    return src.reshape(n, Hs, Ws, 3)


def _numpy_batch(src, rows, cols):
    """The reference's host path: np.array(img, dtype=np.float32) / 255., crop, stack, transpose."""
    imgs = [np.array(src[i], dtype=np.float32) / 255. for i in range(src.shape[0])]
    imgs = [im[np.asarray(rows)][:, np.asarray(cols)] for im in imgs]
    return np.ascontiguousarray(np.stack(imgs).transpose([0, 3, 1, 2]))


def _check(src, rows, cols):
    from cds_mvsnet_amd import ops
    junk = [torch.empty(k, device=DEV) for k in (3, 1001, 77)]          # a used allocator
    del junk[1]
    dsrc = torch.from_numpy(src).to(DEV)
    r, c = ops.index_tables(rows, cols, src.shape[1], src.shape[2], DEV)
    got = ops.image_batch(dsrc, r, c)
    want = torch.from_numpy(_numpy_batch(src, rows, cols))
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.image_batch(dsrc, rows.tolist(), cols.tolist()).cpu(), want)      # host tables are checked and uploaded inside


def test_image_batch_every_byte_value():
    p = np.arange(256)
    src = np.stack([(p * 7 + 85 * c) % 256 for c in range(3)], axis=-1).astype(np.uint8).reshape(1, 16, 16, 3)
    from cds_mvsnet_amd import ops
    got = ops.image_batch(torch.from_numpy(src).to(DEV), np.arange(16), np.arange(16)).cpu()
    assert torch.equal(got, torch.from_numpy(_numpy_batch(src, np.arange(16), np.arange(16))))
    for c in range(3):
        assert len(torch.unique(got[0, c])) == 256
    # what the division is NOT: the multiplication by the rounded reciprocal differs in the last bit for many byte values
    recip = (np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0))
    assert np.count_nonzero(recip != np.arange(256, dtype=np.float32) / 255.) > 100


@pytest.mark.parametrize("shape,origin,size", [((1, 9, 7), (0, 0), (9, 7)),            # whole image, w % 4 != 0
                                               ((1, 37, 53), (2, 3), (32, 48)),          # the aligned vector path, odd origin
                                               ((5, 37, 53), (1, 2), (33, 50)),          # n = 5, scalar stores, several workgroups
                                               ((2, 16, 16), (3, 5), (8, 3))])           # narrower than one vector
def test_image_batch_crops(shape, origin, size):
    src = _source(*shape, seed=sum(shape))
    rows = np.arange(origin[0], origin[0] + size[0])
    cols = np.arange(origin[1], origin[1] + size[1])
    _check(src, rows, cols)


def test_image_batch_strided_tables():
    src = _source(5, 37, 53, seed=9)
    _check(src, np.arange(0, 37, 2)[:16], np.arange(1, 49, 2))        # 16 x 24: the vector path through a gather
    _check(src, np.arange(36, -1, -2), np.arange(1, 53, 2)[:21])      # descending rows, 19 x 21


def test_image_batch_errors():
    from cds_mvsnet_amd import ops
    src = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV)
    r, c = ops.index_tables(np.arange(8), np.arange(8), 8, 8, DEV)
    assert ops.image_batch(src, r, c).shape == (2, 3, 8, 8)
    bad = [(src.float(), r, c),                                # wrong dtype
           (src[0], r, c), (src[..., :2], r, c),               # wrong rank / not 3 channels
           (src.cpu(), r, c),                                  # host tensor
           (src, r.cpu(), c), (src, r, np.arange(8)),          # tables on two sides
           (src, r.long(), c.long()),                          # not int32
           (src, r.view(2, 4), c),
           (src, np.arange(9), np.arange(8)), (src, [0, -1], [0, 1]),      # an index outside the source
           (src.transpose(1, 2), r, c)]                        # not contiguous
    if torch.cuda.device_count() > 1:
        bad.append((src, r.to("cuda:1"), c.to("cuda:1")))      # tables on another device
    for args in bad:
        with pytest.raises(ValueError):
            ops.image_batch(*args)


# ---- a batch against the restatement ------------------------------------------------------------------------------------------------
def _dataset(layout, root, mode, nviews, crop, ndepths=192, interval_scale=1.06, seed=0, **tree):
    from cds_mvsnet_amd import train_data as TD
    if layout == "dtu":
        lst = TR.write_dtu_tree(root, **tree)
        return TD.DTUTrainScenes(str(root), lst, mode, nviews, ndepths, interval_scale, crop=crop, seed=seed), lst
    lst = TR.write_blended_tree(root, **tree)
    return TD.BlendedTrainScenes(str(root), lst, mode, nviews, ndepths, interval_scale, crop=crop, seed=seed), lst


def _assert_batch_equal(got, want):
    assert torch.equal(got["imgs"].cpu(), want["imgs"])
    for k in TR.STAGES:
        assert got["depth"][k].is_cuda and got["mask"][k].is_cuda and got["imgs"].is_cuda
        assert torch.equal(got["depth"][k].cpu(), want["depth"][k]), k
        assert torch.equal(got["mask"][k].cpu(), want["mask"][k]), k
        assert torch.equal(got["proj_matrices"][k].cpu(), want["proj_matrices"][k]), k
    assert torch.equal(got["depth_values"].cpu(), want["depth_values"])
    assert got["filename"] == want["filename"]


@pytest.mark.parametrize("layout", ["dtu", "blended"])
def test_batch_equals_the_restatement(layout, tmp_path):
    from cds_mvsnet_amd import train_data as TD
    crop, B, N, epoch, seed = (64, 96), 2, 3, 1, 5
    if layout == "dtu":                                        # halving 150 x 210 gives 75 x 105, cropped at (5, 4)
        ds, lst = _dataset("dtu", tmp_path, "train", N, crop, seed=seed, n_views=3, image_hw=(64, 96), gt_hw=(150, 210))
        metas = TR.dtu_metas(str(tmp_path), lst)
    else:                                                      # 72 x 104 cropped at (4, 4)
        ds, lst = _dataset("blended", tmp_path, "train", N, crop, seed=seed, n_views=5, image_hw=(72, 104))
        metas = TR.blended_metas(str(tmp_path), lst, N)
    with TD.TrainBatches(ds, B, DEV, epoch=epoch, ahead=0) as it:
        order = [list(b) for b in it.batches]
        assert len(order) == len(ds) // B
        for k, got in zip(range(2), it):
            want = TR.collate([TR.sample(layout, str(tmp_path), metas, i, "train", N, 192, 1.06, crop, seed, epoch) for i in order[k]])
            assert tuple(got["imgs"].shape) == (B, N, 3, 64, 96) and tuple(got["mask"]["stage1"].shape) == (B, 8, 12)
            for name in TR.STAGES:                             # the comparison is not about an empty (or a full) mask
                m = want["mask"][name]
                assert 0 < int(m.sum()) < m.numel(), name
            _assert_batch_equal(got, want)
            assert not got["proj_matrices"]["stage1"].is_cuda and not got["depth_values"].is_cuda      # where train_step wants them


def test_dtu_image_of_another_size_raises(tmp_path):
    from cds_mvsnet_amd import train_data as TD
    ds, _ = _dataset("dtu", tmp_path, "val", 3, (64, 96), n_views=3, image_hw=(66, 96), gt_hw=(150, 210))
    with pytest.raises(ValueError, match="ground-truth crop"):
        next(TD.TrainBatches(ds, 1, DEV, ahead=0))


# ---- decode ahead ------------------------------------------------------------------------------------------------------------------
def _busy(buf, n=100):
    """Queue ~10 ms of memory traffic on the current stream: what follows in the stream (the loader's copy) starts late, as it does
    behind a training step."""
    for _ in range(n):
        buf.add_(1.0)


def _epoch(ds, ahead, threads, busy):
    from cds_mvsnet_amd import train_data as TD
    out = []
    with TD.TrainBatches(ds, 1, DEV, epoch=2, threads=threads, ahead=ahead) as it:
        assert len(it) == 7
        for sample in it:
            _busy(busy)
            out.append(sample)
    torch.cuda.synchronize()
    return out


def test_prefetch_equals_synchronous(tmp_path):
    """7 batches of one sample over a ring of 3 staging buffers: every buffer is refilled at least twice while the stream is kept busy,
    so a buffer handed back to the decoders before its copy has run shows up as another batch's pixels."""
    pairs = [(v, [s for s in range(7) if s != v]) for v in range(7)]
    ds, _ = _dataset("blended", tmp_path, "train", 3, (64, 96), seed=2, n_views=7, pairs=pairs, image_hw=(72, 104))
    busy = torch.zeros(64 << 20, device=DEV)
    start = threading.active_count()
    want = _epoch(ds, 0, 1, busy)
    assert len({s["filename"][0] for s in want}) == 7
    for _ in range(2):
        got = _epoch(ds, 2, 4, busy)
        assert len(got) == len(want) == 7
        for g, w in zip(got, want):
            _assert_batch_equal(g, {k: ({n: t.cpu() for n, t in v.items()} if isinstance(v, dict) else (v.cpu() if torch.is_tensor(v) else v))
                                    for k, v in w.items()})
        assert threading.active_count() == start              # exhaustion shut the pool down


def _close_bounded(it):
    t = threading.Thread(target=it.close)
    t.start()
    t.join(timeout=20)
    assert not t.is_alive(), "TrainBatches.close() did not return"


def test_shutdown(tmp_path):
    from PIL import Image
    from cds_mvsnet_amd import train_data as TD
    pairs = [(v, [s for s in range(7) if s != v]) for v in range(7)]
    ds, _ = _dataset("blended", tmp_path, "val", 3, (64, 96), n_views=7, pairs=pairs, image_hw=(72, 104))
    start = threading.active_count()
    it = TD.TrainBatches(ds, 1, DEV, threads=4, ahead=2)
    first = next(it)                                          # abandoned midway
    assert first["imgs"].shape == (1, 3, 3, 64, 96) and threading.active_count() > start
    _close_bounded(it)
    assert threading.active_count() == start
    with pytest.raises(StopIteration):
        next(it)
    # a worker's exception: the reference image of the fourth batch is grayscale
    bad = os.path.join(str(tmp_path), "sceneA/blended_images/00000003.jpg")
    Image.fromarray(np.full((72, 104), 90, np.uint8)).save(bad)
    ds2 = TD.BlendedTrainScenes(str(tmp_path), ds.listfile, "val", 2, crop=(64, 96))    # 2 views: batch k reads views k and 0 (or 1)
    it = TD.TrainBatches(ds2, 1, DEV, threads=4, ahead=2)
    with pytest.raises(ValueError) as e:
        for _ in range(7):
            next(it)
    assert bad in str(e.value)
    _close_bounded(it)
    assert threading.active_count() == start
    torch.cuda.synchronize()


# ---- fit ---------------------------------------------------------------------------------------------------------------------------
def test_fit_end_to_end(tmp_path, seeded_state):
    from cds_mvsnet_amd import depth_eval, fit, infer
    from cds_mvsnet_amd import train as T
    from cds_mvsnet_amd import train_data as TD
    root, crop, N, B = str(tmp_path / "data"), (128, 192), 3, 2
    os.makedirs(root)
    four = [(v, [s for s in range(4) if s != v]) for v in range(4)]
    trainlist = TR.write_blended_tree(root, scans=("sceneA",), n_views=4, pairs=four, image_hw=(136, 200), seed=1, listname="train.txt")
    vallist = TR.write_blended_tree(root, scans=("sceneV",), n_views=3, pairs=[(0, [1, 2]), (1, [0, 2])], image_hw=(136, 200), seed=2,
                                    listname="val.txt")
    train_ds = TD.BlendedTrainScenes(root, trainlist, "train", N, 192, 1.0, crop=crop)
    val_ds = TD.BlendedTrainScenes(root, vallist, "val", N, 192, 1.0, crop=crop)
    assert len(train_ds) == 4 and len(val_ds) == 2
    save = str(tmp_path / "saved")
    lines = []
    model = seeded_state(True).to(DEV)
    start = threading.active_count()
    log = fit.fit(model, [train_ds], [val_ds], epochs=2, batch_size=B, val_batch_size=1, eval_freq=1, save_period=1, save_dir=save,
                  logging_every=1, monitor="min abs_depth_error", config={"arch": {"type": "CDSMVSNet"}}, log=lines.append)
    assert threading.active_count() == start
    assert [r["epoch"] for r in log] == [1, 2] and [r["steps"] for r in log] == [2, 2]
    assert log[0]["temperature"] == 1.0 and log[1]["temperature"] == 10 ** -0.5
    assert log[0]["lr"] == log[1]["lr"] == 1e-4               # StepLR(3) has not fired
    for r in log:
        assert math.isfinite(r["loss"]) and math.isfinite(r["depth_loss"]) and r["depth_loss"] > 0
        assert [x[0] for x in r["logged"]] == [0, 1] and all(math.isfinite(v) for x in r["logged"] for v in x)
        assert abs(sum(x[1] for x in r["logged"]) / 2 - r["loss"]) <= 1e-6 * abs(r["loss"])
        assert list(r["val"]) == ["loss", "depth_loss"] + list(depth_eval.VALIDATION_NAMES) and len(depth_eval.VALIDATION_NAMES) == 12
        assert all(math.isfinite(v) for v in r["val"].values())
    assert any(ln.startswith("Epoch 1/2, Iter 0/2, lr 0.000100, train loss = ") for ln in lines)
    import json
    with open(os.path.join(save, "log.json")) as f:
        assert json.load(f) == json.loads(json.dumps(log))

    # the first step by hand: the same seeded weights on the restatement's first batch
    metas = TR.blended_metas(root, trainlist, N)
    first = TD.epoch_batches(4, B, seed=0, epoch=1)[0]
    want = TR.collate([TR.sample("blended", root, metas, i, "train", N, 192, 1.0, crop, 0, 1) for i in first])
    sample = {"imgs": want["imgs"].to(DEV), "proj_matrices": want["proj_matrices"], "depth_values": want["depth_values"],
              "depth": {k: v.to(DEV) for k, v in want["depth"].items()}, "mask": {k: v.to(DEV) for k, v in want["mask"].items()}}
    hand = seeded_state(True).to(DEV)
    loss, depth_loss = T.train_step(hand, T.make_optimizer(hand), sample, temperature=1.0)
    assert log[0]["logged"][0][1] == pytest.approx(loss, rel=1e-6)
    assert log[0]["logged"][0][2] == pytest.approx(depth_loss, rel=1e-6)

    # checkpoints
    for name in ("checkpoint-epoch1.pth", "checkpoint-epoch2.pth", "model_best.pth"):
        path = os.path.join(save, name)
        assert os.path.isfile(path), name
        ck = torch.load(path, map_location="cpu", weights_only=True)
        assert tuple(ck) == fit.CHECKPOINT_KEYS
        infer.load_checkpoint(seeded_state(True), path)
    last = torch.load(os.path.join(save, "checkpoint-epoch2.pth"), map_location="cpu", weights_only=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), last["state_dict"][k]), k
    assert last["monitor_best"] == min(r["val"]["abs_depth_error"] for r in log)

    # resume from epoch 1: exactly epoch 2
    again = seeded_state(True).to(DEV)
    save2 = str(tmp_path / "saved2")
    log2 = fit.fit(again, [train_ds], [val_ds], epochs=2, batch_size=B, eval_freq=1, save_period=1, save_dir=save2, logging_every=1,
                   monitor="min abs_depth_error", resume=os.path.join(save, "checkpoint-epoch1.pth"), log=lines.append)
    assert [r["epoch"] for r in log2] == [2] and log2[0]["steps"] == 2
    assert log2[0]["temperature"] == 10 ** -0.5 and log2[0]["lr"] == 1e-4
    assert os.listdir(save2).count("checkpoint-epoch2.pth") == 1 and not os.path.exists(os.path.join(save2, "checkpoint-epoch1.pth"))
    assert log2[0]["logged"][0][1] == pytest.approx(log[1]["logged"][0][1], rel=1e-6)     # the same weights, batch, temperature: the same forward
