"""Depth-map evaluation on the GPU (csrc/depth_metrics.hip, cds_mvsnet_amd/depth_eval.py) against the float64 restatement of
tests/depth_eval_ref.py and the reference's own numbers (golden set G16).

Tolerances: pixel COUNTS must be equal; fp64 SUMS within rel 1e-9 (an fp64 sum of <= 2^20 terms of one sign is within n 2^-53
~ 1e-10 of the exact sum whatever the order); scalars against the REFERENCE's float32 means within rel n 2^-24 = 2.5e-4 for
n <= 4096 masked pixels (the worst case of any float32 summation order)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import depth_eval_ref as R
from conftest import GOLDEN
from test_mvs_io import _write_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL_SUM = 1e-9
REL_REF = 4096 * 2.0 ** -24


def _g16():
    z = np.load(os.path.join(GOLDEN, "g16_depth_metrics.npz"))
    return {k: z[k] for k in z.files}


def _inputs(B, h, w, T, seed, thr_per_image=False):
    """est, gt, mask, thr: errors spread over all bands, a few pixels exactly on / one ulp either side of every threshold (gt = 0
    there, so e is that float32 bit for bit), mask values 0, 0.5 (not selected), 0.75 and 1."""
    rs = np.random.RandomState(seed)
    thr = np.sort(rs.rand(B if thr_per_image else 1, T) * 8 + 0.1, axis=1).astype(np.float32)
    gt = (rs.rand(B, h, w) * 400 + 450).astype(np.float32)
    est = (gt + (rs.rand(B, h, w) * 10 - 5).astype(np.float32) * (rs.rand(B, h, w) < 0.9)).astype(np.float32)
    mask = rs.choice(np.array([0.0, 0.5, 0.75, 1.0], np.float32), size=(B, h, w), p=[0.25, 0.05, 0.1, 0.6])
    flat = rs.permutation(h * w)
    k = 0
    for b in range(B):
        for t in thr[b if thr_per_image else 0]:
            for v in (np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(np.inf))):
                if k >= flat.size:
                    break
                y, x = divmod(int(flat[k]), w)
                k += 1
                est[b, y, x], gt[b, y, x], mask[b, y, x] = v, 0.0, 1.0
    return est, gt, mask, (thr if thr_per_image else thr[0])


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _check_sums(got, want, T):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64
    counts = [0] + list(range(3, 3 + T)) + list(range(3 + T, 3 * T + 5, 2))
    sums = [1, 2] + list(range(4 + T, 3 * T + 5, 2))
    assert np.array_equal(got[:, counts], want[:, counts]), (got[:, counts], want[:, counts])
    for f in sums:
        for b in range(got.shape[0]):
            g, w = got[b, f], want[b, f]
            assert (g == 0.0 if w == 0.0 else abs(g - w) <= REL_SUM * abs(w)), (b, f, g, w)


def _shift4(t):
    """The same values in storage that starts 4 bytes past a 16-byte boundary: the kernel must take its scalar loads."""
    out = torch.cat((torch.zeros(1, device=DEV), t.reshape(-1)))[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.mark.parametrize("B,h,w,T,shifted", [(1, 1, 1, 0, False), (1, 5, 7, 1, False), (3, 5, 7, 5, False), (2, 48, 64, 8, False),
                                             (2, 520, 520, 5, False), (2, 520, 520, 5, True), (2, 760, 760, 5, False)])
def test_metric_sums_match_the_restatement(B, h, w, T, shifted):
    """The first pass runs 512 workgroups x 256 threads = 131 072 lanes per image at B = 2, each striding by that number.
    (2, 520, 520, 5): 270 400 pixels per image; aligned storage reads them as 67 600 float4 (ONE trip of the vector loop, half the
    lanes idle), the storage shifted by 4 bytes as scalars (THREE trips of the scalar loop, the last one partial).
    (2, 760, 760, 5): 144 400 float4 per image, TWO trips of the vector loop, the second partial.
    (3, 5, 7, 5): images 1 and 2 start at offsets 35 and 70, no multiple of 4 (scalar loads), image 0 reads float4 + a 3-pixel tail."""
    from cds_mvsnet_amd import ops
    if B == 2 and h >= 520:
        trips = -(-(h * w if shifted else h * w // 4) // (512 * 256))
        assert trips == {(520, False): 1, (520, True): 3, (760, False): 2}[(h, shifted)]
    est, gt, mask, thr = _inputs(B, h, w, T, seed=100 + h)
    d = _dev(est, gt, mask)
    if shifted:
        d = [_shift4(t) for t in d]
    else:
        assert all(t.data_ptr() % 16 == 0 for t in d)
    a = ops.depth_metric_sums(*d, thr, 1e5)
    b = ops.depth_metric_sums(*d, thr, 1e5)
    assert a.shape == (B, 3 * T + 5) and a.dtype == torch.float64 and a.is_cuda
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))              # bit-identical run to run
    _check_sums(a, R.metric_sums(est, gt, mask, thr, 1e5), T)


def test_metric_sums_edge_cases():
    from cds_mvsnet_amd import ops
    g = _g16()
    # the G16 inputs: pixels exactly on the float32 thresholds
    di = float(g["a_interval"][0]) / 2.65
    thr = [di * m for m in R.MULTIPLIERS]
    d = _dev(g["a_est"], g["a_gt"], g["a_mask"])
    _check_sums(ops.depth_metric_sums(*d, thr, R.CAP), R.metric_sums(g["a_est"], g["a_gt"], g["a_mask"], thr, R.CAP), 5)
    # an empty mask beside one that is not; a small cap (errors above it are in no band)
    est, gt, mask, thr = _inputs(3, 9, 11, 3, seed=5)
    mask[1] = 0.0
    got = ops.depth_metric_sums(*_dev(est, gt, mask), thr, 3.0)
    _check_sums(got, R.metric_sums(est, gt, mask, thr, 3.0), 3)
    assert (got[1] == 0).all() and got[0, 0] > 0 and got[2, 0] > 0
    # per-image thresholds, from the host and as a device tensor
    est, gt, mask, thr = _inputs(3, 17, 13, 4, seed=6, thr_per_image=True)
    want = R.metric_sums(est, gt, mask, thr, 1e5)
    assert not np.array_equal(want[0, 3:7], want[1, 3:7])
    _check_sums(ops.depth_metric_sums(*_dev(est, gt, mask), thr, 1e5), want, 4)
    _check_sums(ops.depth_metric_sums(*_dev(est, gt, mask), torch.from_numpy(thr).to(DEV), 1e5), want, 4)
    # tensors whose storage offset breaks the 16-byte alignment take the scalar loads
    est, gt, mask, thr = _inputs(2, 6, 8, 2, seed=7)
    shifted = [_shift4(t) for t in _dev(est, gt, mask)]
    _check_sums(ops.depth_metric_sums(*shifted, thr, 1e5), R.metric_sums(est, gt, mask, thr, 1e5), 2)
    # a NaN estimate under the mask: counted, poisons the two sums, exceeds nothing, lies in no band
    est, gt, mask, thr = _inputs(1, 4, 4, 2, seed=8)
    mask[:] = 1.0
    est[0, 2, 2] = np.nan
    got = ops.depth_metric_sums(*_dev(est, gt, mask), thr, 1e5).cpu().numpy()
    want = R.metric_sums(est, gt, mask, thr, 1e5)
    assert got[0, 0] == 16 and math.isnan(got[0, 1]) and math.isnan(got[0, 2])
    assert np.array_equal(got[0, 3:5], want[0, 3:5]) and np.array_equal(got[0, 5::2], want[0, 5::2])
    assert got[0, 5::2].sum() >= 15 and np.isfinite(got[0, 6::2]).all()


def test_metric_sums_refuse_bad_arguments():
    from cds_mvsnet_amd import ops
    x = torch.zeros(2, 4, 4, device=DEV)
    with pytest.raises(RuntimeError):
        ops.depth_metric_sums(x.cpu(), x, x, [1.0], 1e5)
    with pytest.raises(ValueError):
        ops.depth_metric_sums(x, x[:1], x, [1.0], 1e5)
    with pytest.raises(ValueError):
        ops.depth_metric_sums(x[0], x[0], x[0], [1.0], 1e5)
    with pytest.raises(ValueError, match="ascend"):
        ops.depth_metric_sums(x, x, x, [2.0, 1.0], 1e5)
    with pytest.raises(ValueError, match="at most 8"):
        ops.depth_metric_sums(x, x, x, list(range(9)), 1e5)
    with pytest.raises(ValueError):
        ops.depth_metric_sums(x, x, x, np.ones((3, 2)), 1e5)
    with pytest.raises(TypeError):
        ops.depth_metric_sums(x.double(), x, x, [1.0], 1e5)
    assert ops.depth_metric_sums(x, x, x, [1.0, 1.0], 1e5).shape == (2, 11)     # equal thresholds ascend


def test_scalars_against_the_reference():
    """validation_scalars / precision_scalars on the G16 inputs against what the reference's own functions returned."""
    from cds_mvsnet_amd import depth_eval as E
    g = _g16()
    for tag in ("a", "b"):
        est, gt, mask = _dev(g[f"{tag}_est"], g[f"{tag}_gt"], g[f"{tag}_mask"])
        assert max(int((m > 0.5).sum()) for m in g[f"{tag}_mask"]) <= 4096
        for interval in (g[f"{tag}_interval"], torch.from_numpy(g[f"{tag}_interval"]).to(DEV)):     # host and device di
            got = E.validation_scalars({"refined_depth": est}, {"stage4": gt}, {"stage4": mask}, interval)
            assert tuple(got) == R.NAMES
            for k, want in zip(R.NAMES, g[f"{tag}_validation"]):
                assert (math.isnan(got[k]) if math.isnan(want) else abs(got[k] - want) <= REL_REF * abs(want)), (tag, k, got[k], want)
        gotp = E.precision_scalars(est, gt, mask > 0.5)                                              # a bool mask is accepted
        for k, want in zip(R.PRECISION_NAMES, g[f"{tag}_precision"]):
            assert (math.isnan(gotp[k]) if math.isnan(want) else abs(gotp[k] - want) <= REL_REF * abs(want)), (tag, k, gotp[k], want)
    est, gt, mask = _dev(g["a_est"], g["a_gt"], g["a_mask"])
    m = E.depth_metrics(est, gt, mask, [1.0, 2.0, 4.0])
    want = R.precision_scalars(g["a_est"], g["a_gt"], g["a_mask"])
    assert abs(m["abs_depth_error"] - want["MAE"]) <= REL_SUM * want["MAE"] and abs(m["rmse"] - want["RMSE"]) <= REL_SUM * want["RMSE"]
    assert len(m["thres_error"]) == 3 and len(m["band_abserror"]) == 4 and m["pixels"] == [int((x > 0.5).sum()) for x in g["a_mask"]]
    assert abs((1.0 - m["thres_error"][1]) - want["thresh2mm_error"]) < 1e-12


# ---- kernel B ------------------------------------------------------------------------------------------------------------------------
def _check_pyramid(got, want):
    (gd, gm), (wd, wm) = got, want
    assert len(gd) == len(wd) == len(gm) == len(wm)
    for a, b in zip(gd + gm, wd + wm):
        a = a.cpu().numpy()
        assert a.shape == b.shape and a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_gt_pyramid_dtu_rule(tmp_path):
    from PIL import Image
    from cds_mvsnet_amd import depth_eval as E, mvs_io, ops
    rs = np.random.RandomState(1)
    src = (rs.rand(40, 48) * 400 + 450).astype(np.float32)
    m8 = rs.choice(np.array([0, 9, 10, 11, 255], np.uint8), size=(40, 48))
    rows, cols = R.dtu_tables(40, 48, (16, 16))                    # halve to 20 x 24, crop 16 x 16 from (2, 4)
    assert rows[0] == 4 and cols[0] == 8 and {9, 10, 11} <= set(m8[rows][:, cols].reshape(-1).tolist())
    want = R.pyramid(src, rows, cols, 4, m8, 10)
    assert [d.shape for d in want[0]] == [(16, 16), (8, 8), (4, 4), (2, 2)]
    d, m = _dev(src, m8)
    _check_pyramid(ops.gt_pyramid(d, rows, cols, levels=4, mask_src=m, mask_thresh=10), want)
    # the same through the files
    mvs_io.write_pfm(str(tmp_path / "d.pfm"), src)
    Image.fromarray(m8).save(tmp_path / "m.png")
    depth_ms, mask_ms = E.read_gt_ms(str(tmp_path / "d.pfm"), str(tmp_path / "m.png"), "dtu", DEV, crop=(16, 16))
    assert list(depth_ms) == ["stage4", "stage3", "stage2", "stage1"]
    _check_pyramid(([depth_ms[f"stage{k}"] for k in (4, 3, 2, 1)], [mask_ms[f"stage{k}"] for k in (4, 3, 2, 1)]), want)
    # a table cache kept by the caller: filled by the first view, reused by the second
    cache = {}
    for _ in range(2):
        depth_ms, mask_ms = E.read_gt_ms(str(tmp_path / "d.pfm"), str(tmp_path / "m.png"), "dtu", DEV, crop=(16, 16), tables=cache)
        _check_pyramid(([depth_ms[f"stage{k}"] for k in (4, 3, 2, 1)], [mask_ms[f"stage{k}"] for k in (4, 3, 2, 1)]), want)
        assert len(cache) == 1
    with pytest.raises(ValueError):
        E.read_gt_ms(str(tmp_path / "d.pfm"), None, "dtu", DEV, crop=(16, 16))


def test_gt_pyramid_blended_rule_and_resize(tmp_path):
    from cds_mvsnet_amd import depth_eval as E, mvs_io, ops
    rs = np.random.RandomState(2)
    src = rs.choice(np.array([0.0, -1.0, 1e-30, 3.5, 712.25], np.float32), size=(41, 49))
    rows, cols = R.blended_tables(41, 49, (16, 32))
    assert rows[0] == 12 and cols[0] == 8
    want = R.pyramid(src, rows, cols, 3)
    lvl0 = src[rows][:, cols]
    assert all((lvl0 == np.float32(v)).any() for v in (0.0, -1.0, 1e-30)) and np.array_equal(want[1][0], (lvl0 > 0).astype(np.float32))
    assert want[1][0][lvl0 == np.float32(1e-30)].all() and not want[1][0][lvl0 <= 0].any()
    mvs_io.write_pfm(str(tmp_path / "d.pfm"), src)
    depth_ms, mask_ms = E.read_gt_ms(str(tmp_path / "d.pfm"), None, "blended", DEV, levels=3, crop=(16, 32))
    _check_pyramid(([depth_ms[f"stage{k}"] for k in (3, 2, 1)], [mask_ms[f"stage{k}"] for k in (3, 2, 1)]), want)
    # a non-integer resize through nearest_index, 21 x 37 -> 8 x 16
    src = (rs.rand(21, 37) * 100).astype(np.float32)
    rows, cols = E.resize_tables(21, 37, 8, 16)
    assert np.array_equal(rows, R.nearest_index(8, 21)) and np.array_equal(cols, R.nearest_index(16, 37))
    _check_pyramid(ops.gt_pyramid(_dev(src)[0], rows, cols, levels=4), R.pyramid(src, rows, cols, 4))
    # tables uploaded once (ops.index_tables) serve many calls; the result is the same
    dr, dc = ops.index_tables(rows, cols, 21, 37, DEV)
    assert dr.is_cuda and dr.dtype == torch.int32 and dc.shape == (16,)
    for seed in (3, 4):
        other = (np.random.RandomState(seed).rand(21, 37) * 100).astype(np.float32)
        _check_pyramid(ops.gt_pyramid(_dev(other)[0], dr, dc, levels=4), R.pyramid(other, rows, cols, 4))
    with pytest.raises(ValueError):
        ops.gt_pyramid(_dev(src)[0], dr, cols, levels=4)                      # one table on the device, one on the host
    with pytest.raises(ValueError):
        ops.gt_pyramid(_dev(src)[0], dr.long(), dc.long(), levels=4)
    # sizes that the levels do not divide, and tables that leave the source
    d = _dev(src)[0]
    with pytest.raises(ValueError, match="multiple"):
        ops.gt_pyramid(d, np.arange(12), np.arange(16), levels=4)
    assert len(ops.gt_pyramid(d, np.arange(12), np.arange(16), levels=3)[0]) == 3
    with pytest.raises(ValueError, match="outside"):
        ops.gt_pyramid(d, [0, 21], [0, 1], levels=1)
    with pytest.raises(ValueError, match="outside"):
        ops.gt_pyramid(d, [0, 1], [-1, 1], levels=1)
    with pytest.raises(ValueError):
        ops.gt_pyramid(d, [0, 1], [0, 1], levels=5)


# ---- validate() ----------------------------------------------------------------------------------------------------------------------
def _sample(seed, N=3, H=128, W=192):
    """A refine=True sample: 128 x 192 images, the three stages at 16 x 24, 32 x 48, 64 x 96 (the model's internal resolution is half
    the image's and must be a multiple of 32), stage4 at the image size; <= 4096 masked pixels at stage4."""
    from cds_mvsnet_amd import synth
    g = torch.Generator().manual_seed(seed)
    full = 500.0 + 250.0 * torch.rand(1, H // 8, W // 8, generator=g)
    full = torch.nn.functional.interpolate(full[None], (H, W), mode="bilinear", align_corners=False)[0]
    sample = {"imgs": synth.make_images(N, H, W, seed=seed).to(DEV),
              "proj_matrices": {k: v.to(DEV) for k, v in synth.make_cameras(N, H, W, refine=True, seed=seed).items()},
              "depth_values": synth.make_depth_values().to(DEV), "depth": {}, "mask": {}}
    for k, step in (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1)):
        sample["depth"][k] = full[:, ::step, ::step].contiguous().to(DEV)
        keep = 0.9 if step > 1 else 0.15
        sample["mask"][k] = (torch.rand(1, H // step, W // step, generator=g) < keep).float().to(DEV)
    assert int(sample["mask"]["stage4"].sum()) <= 4096
    return sample


def test_validate_equals_the_sample_by_sample_formulation(seeded_state):
    from cds_mvsnet_amd import depth_eval as E
    from cds_mvsnet_amd.losses import final_loss
    model = seeded_state(True).to(DEV)
    samples = [_sample(31), _sample(32)]
    dlossw = [0.5, 1.0, 2.0]
    T = 0.01
    want = {}
    with torch.no_grad():
        for s in samples:
            out = model(s["imgs"], s["proj_matrices"], s["depth_values"], temperature=T)
            interval = s["depth_values"][:, 1] - s["depth_values"][:, 0]
            loss, dl = final_loss(out, s["depth"], s["mask"], dlossw=dlossw, depth_interval=interval)
            sc = {"loss": float(loss), "depth_loss": float(dl)}
            sc.update(R.torch_validation_scalars(out["refined_depth"], s["depth"]["stage4"], s["mask"]["stage4"], interval))
            for k, v in sc.items():
                want[k] = want.get(k, 0.0) + v / len(samples)
    got = E.validate(model, iter(samples), T, dlossw=dlossw)
    assert list(got) == ["loss", "depth_loss"] + list(R.NAMES) and not model.training
    for k in got:
        rel = 1e-6 if k in ("loss", "depth_loss") else REL_REF
        assert math.isfinite(want[k]) and abs(got[k] - want[k]) <= rel * abs(want[k]), (k, got[k], want[k])
    assert got["abs_depth_error"] > 0 and 0 < got["thres2mm_error"] <= 1
    # the mode is restored; a sample with an empty stage-4 mask makes the means over the mask NaN, as in the reference
    model.train()
    empty = dict(samples[1], mask=dict(samples[1]["mask"], stage4=torch.zeros_like(samples[1]["mask"]["stage4"])))
    got2 = E.validate(model, [samples[0], empty], T, dlossw=dlossw)
    assert model.training
    model.eval()
    for k in ("abs_depth_error", "thres2mm_error", "thres20mm_error", "loss"):
        assert math.isnan(got2[k]), k
    one = E.validate(model, [samples[0]], T, dlossw=dlossw)
    for k in R.NAMES[6:]:                                          # the empty sample's bands are 0: half the first sample's value
        assert abs(got2[k] - one[k] / 2) <= 1e-12 * abs(one[k]), k
    with pytest.raises(ValueError):
        E.validate(model, [], T)


# ---- command lines -------------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path):
    from PIL import Image
    from cds_mvsnet_amd import depth_eval as E, mvs_io
    rs = np.random.RandomState(3)
    gtdir, outdir = tmp_path / "Depths_raw", tmp_path / "out"
    want = {"depth_est": [], "depth_stage3": []}
    rows, cols = R.nearest_index(40, 80), R.nearest_index(48, 96)
    for scan in ("scan1", "scan9"):
        os.makedirs(gtdir / scan)
        for folder in want:
            os.makedirs(outdir / scan / folder)
        for v in range(3):
            gt = (rs.rand(80, 96) * 400 + 450).astype(np.float32)
            m8 = rs.choice(np.array([0, 9, 10, 11, 200], np.uint8), size=(80, 96))
            mvs_io.write_pfm(str(gtdir / scan / f"depth_map_{v:04d}.pfm"), gt)
            Image.fromarray(m8).save(gtdir / scan / f"depth_visual_{v:04d}.png")
            (d,), (m,) = R.pyramid(gt, rows, cols, 1, m8, 10)
            for folder, noise in (("depth_est", 1.5), ("depth_stage3", 4.0)):
                est = (d + rs.randn(40, 48).astype(np.float32) * np.float32(noise)).astype(np.float32)
                est[0, :3] = d[0, :3] + np.array([1.0, 2.0, 4.0], np.float32)
                mvs_io.write_pfm(str(outdir / scan / folder / f"{v:08d}.pfm"), est)
                want[folder].append(R.precision_scalars(est, d, m))
    with open(tmp_path / "list.txt", "w") as f:
        f.write("scan1\nscan9\n")
    argv = ["--gtpath", str(gtdir), "--outdir", str(outdir), "--testlist", str(tmp_path / "list.txt"),
            "--folders", "depth_est,depth_stage3", "--json", str(tmp_path / "res.json")]
    res = E.main(argv)
    assert json.load(open(tmp_path / "res.json")) == res and list(res["folders"]) == ["depth_est", "depth_stage3"]
    for folder, per_image in want.items():
        r = res["folders"][folder]
        assert r["images"] == 6
        for k in R.PRECISION_NAMES:
            w = float(np.mean([p[k] for p in per_image]))
            assert abs(r[k] - w) <= REL_SUM * abs(w), (folder, k, r[k], w)
    assert res["folders"]["depth_est"]["MAE"] < res["folders"]["depth_stage3"]["MAE"]
    os.remove(gtdir / "scan9" / "depth_map_0001.pfm")
    with pytest.raises(FileNotFoundError, match="depth_map_0001.pfm"):
        E.main(argv)


def test_infer_save_stages(tmp_path):
    from cds_mvsnet_amd import infer, mvs_io
    root = str(tmp_path / "scenes")
    os.makedirs(root)
    _write_scene(root, "scanS", 3, 128, 160, seed=3)
    with open(tmp_path / "list.txt", "w") as f:
        f.write("scanS\n")
    base = ["--testpath", root, "--testlist", str(tmp_path / "list.txt"), "--num_view", "3", "--max_h", "128", "--max_w", "160",
            "--interval_scale", "1.0"]
    infer.main(base + ["--outdir", str(tmp_path / "plain")])
    infer.main(base + ["--outdir", str(tmp_path / "stages"), "--save_stages"])
    assert sorted(os.listdir(tmp_path / "plain" / "scanS")) == ["cams", "confidence", "depth_est", "images"]
    assert sorted(os.listdir(tmp_path / "stages" / "scanS")) == ["cams", "confidence", "depth_est", "depth_stage1", "depth_stage2",
                                                                   "depth_stage3", "images"]
    for v in range(3):
        name = f"{v:08d}.pfm"
        assert open(tmp_path / "plain" / "scanS" / "depth_est" / name, "rb").read() == \
            open(tmp_path / "stages" / "scanS" / "depth_est" / name, "rb").read()
        for k, shape in ((1, (32, 40)), (2, (64, 80)), (3, (128, 160))):
            d = mvs_io.read_pfm(str(tmp_path / "stages" / "scanS" / f"depth_stage{k}" / name))[0]
            assert d.shape == shape and np.isfinite(d).all() and d.min() > 0
        # without the refinement network the last stage IS the estimate
        assert np.array_equal(mvs_io.read_pfm(str(tmp_path / "stages" / "scanS" / "depth_stage3" / name))[0],
                              mvs_io.read_pfm(str(tmp_path / "stages" / "scanS" / "depth_est" / name))[0])
