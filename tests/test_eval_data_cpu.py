"""cds_mvsnet_amd.eval_data without a GPU: the resize tables, the rounding bound of the float32 resize through them (and its equality
with the restatement the GPU tests compare against), the new command-line flags and their way into the model, the view cache and
the output writer's error path."""
import os
import re
import threading

import numpy as np
import pytest
import torch

import eval_data_ref as R
from conftest import ROOT


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def test_tables_equal_sizes_and_upsampling():
    from cds_mvsnet_amd import eval_data as E
    for n in (1, 7, 64):
        s0, s1, f = E.linear_tables(n, n)
        assert np.array_equal(s0, np.arange(n)) and np.array_equal(s1, np.minimum(np.arange(n) + 1, n - 1)) and not f.any()
        assert s0.dtype == s1.dtype == np.int32 and f.dtype == np.float32
    s0, s1, f = E.linear_tables(16, 32)
    assert (s0[0], f[0]) == (0, 0.0)                           # clamped from -0.25
    assert (s0[1], s1[1], f[1]) == (0, 1, 0.25)
    assert (s0[31], s1[31], f[31]) == (15, 15, 0.0)            # 15.25: the last source sample, weight dropped
    assert (s0[30], s1[30], f[30]) == (14, 15, 0.75)


@pytest.mark.parametrize("S,d", [(1200, 1184), (1088, 544), (1920, 1024), (53, 48), (24, 48), (70, 45)])
def test_tables_in_bounds_and_monotonic(S, d):
    from cds_mvsnet_amd import eval_data as E
    s0, s1, f = E.linear_tables(S, d)
    assert s0.min() >= 0 and s1.max() <= S - 1 and np.all(s1 >= s0) and np.all(s1 - s0 <= 1)
    assert np.all(np.diff(s0) >= 0) and np.all(np.diff(s1) >= 0)
    assert np.all((0 <= f) & (f < 1))
    r0, r1, rf = R.taps(S, d)                                  # the loop restatement agrees entry for entry
    assert np.array_equal(s0, r0) and np.array_equal(s1, r1) and np.array_equal(f, rf)


def test_tables_fold_the_edge_padding():
    from cds_mvsnet_amd import eval_data as E
    Hs = 24
    s0, s1, f = E.linear_tables(Hs, Hs + 8, pad=4)             # no resize: padded rows 0..4 -> 0, the last five -> Hs - 1
    assert not f.any()
    assert np.array_equal(s0[:5], np.zeros(5)) and np.array_equal(s0[-5:], np.full(5, Hs - 1))
    assert np.array_equal(s0[4:-4], np.arange(Hs))
    s0, s1, f = E.linear_tables(100, 54, pad=4)                # with a resize: the taps of the padded axis, shifted and clamped
    p0, p1, pf = R.taps(108, 54)
    assert np.array_equal(s0, np.clip(p0 - 4, 0, 99)) and np.array_equal(s1, np.clip(p1 - 4, 0, 99)) and np.array_equal(f, pf)
    with pytest.raises(ValueError):
        E.linear_tables(0, 4)


def test_nearest_tables_are_nearest_resize():
    from cds_mvsnet_amd import eval_data as E
    from cds_mvsnet_amd import mvs_io
    for S, d in ((16, 64), (40, 150), (160, 150), (7, 7)):
        a = np.arange(S * 3, dtype=np.float32).reshape(S, 3)
        assert np.array_equal(a[E.nearest_tables(S, d)], mvs_io.nearest_resize(a, d, 3))


# ---- the restatement and the product's tables ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [((37, 53), (32, 48)), ((16, 24), (32, 48)), ((50, 70), (64, 96)), ((1080, 1920), (544, 1024))])
def test_float32_resize_is_within_its_rounding_bound(src, dst):
    """The product's tables (eval_data.linear_tables, padding folded in) evaluated in float32 and in float64 on the same float32
    ``u8 / 255`` inputs.  Values are at most 1 and the two passes round at most six times (two products and a sum each), 2^-25 apiece at
    most: the float32 result lies within 6 * 2^-25 = 3 * 2^-24 < 2^-22 of float64.  Measured: at most 2.0 * 2^-24 on these shapes.
    The float32 result is also, bit for bit, the restatement's with its own loop-built taps on the padded image - the array the GPU
    tests compare the kernel with."""
    from cds_mvsnet_amd import eval_data as E
    u8 = R.random_u8(src + (3,), seed=src[0])
    pad = 4 if src == (1080, 1920) else 0
    rows, cols = E.linear_tables(src[0], dst[0], pad), E.linear_tables(src[1], dst[1])
    f32 = R.resize_through(u8, rows, cols, np.float32)
    f64 = R.resize_through(u8, rows, cols, np.float64)
    assert f32.dtype == np.float32 and f32.shape == (3,) + dst
    err = float(np.abs(f32.astype(np.float64) - f64).max())
    print(f"{src} -> {dst}: max |f32 - f64| = {err / 2 ** -24:.3f} * 2^-24")
    assert err <= 2.0 ** -22
    assert 0.0 <= f64.min() and f64.max() <= 1.0
    assert np.array_equal(f32, R.resize(u8, dst[0], dst[1], pad, np.float32))
    assert np.array_equal(f64, R.resize(u8, dst[0], dst[1], pad, np.float64))


def test_resize_without_resize_is_the_padded_division():
    from cds_mvsnet_amd import eval_data as E
    u8 = R.random_u8((24, 40, 3), seed=1)
    want = np.pad(np.array(u8, np.float32) / 255., ((4, 4), (0, 0), (0, 0)), "edge").transpose(2, 0, 1)
    assert np.array_equal(R.resize_through(u8, E.linear_tables(24, 32, 4), E.linear_tables(40, 40)), want)
    assert np.array_equal(R.resize(u8, 32, 40, pad=4), want)


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_parse_args_defaults_and_choices(capsys):
    from cds_mvsnet_amd import infer
    base = ["--testpath", "a", "--testlist", "b", "--outdir", "c"]
    a = infer.parse_args(base)
    assert a.pipeline == "host" and a.view_cache_mb == 2048.0
    assert a.ndepths == (48, 32, 8) and a.depth_inter_r == (4.0, 1.5, 0.75)
    b = infer.parse_args(base + ["--pipeline", "gpu", "--view_cache_mb", "100", "--ndepths", "64,32,8", "--depth_inter_r", "4,2,1"])
    assert b.pipeline == "gpu" and b.view_cache_mb == 100.0
    assert b.ndepths == (64, 32, 8) and b.depth_inter_r == (4.0, 2.0, 1.0) and all(isinstance(x, int) for x in b.ndepths)
    for bad in (["--pipeline", "both"], ["--ndepths", "48,32"], ["--ndepths", "48,32,8,4"], ["--ndepths", "a,b,c"],
                ["--ndepths", "4.5,3,1"], ["--depth_inter_r", "4,2"]):
        with pytest.raises(SystemExit):                        # a usage error at parse time
            infer.parse_args(base + bad)
        assert bad[0] in capsys.readouterr().err
    # the help says that the two pipelines differ when an image is resized
    with pytest.raises(SystemExit):
        infer.parse_args(["--help"])
    text = re.sub(r"\s+", " ", capsys.readouterr().out)
    assert "--pipeline" in text and "DIFFER" in text and "INTER_LINEAR" in text


def test_stage_flags_reach_the_model():
    """--ndepths / --depth_inter_r are what CDSMVSNet is built with (each its own, not swapped, not the defaults regardless); the
    defaults build the model infer built before the flags existed."""
    from cds_mvsnet_amd import CDSMVSNet, infer, seeded_init_
    base = ["--testpath", "a", "--testlist", "b", "--outdir", "c"]
    m = infer.build_model(infer.parse_args(base + ["--ndepths", "64,32,8", "--depth_inter_r", "3.0,2.0,0.5", "--refine"]))
    assert m.ndepths == (64, 32, 8) and m.depth_interals_ratio == (3.0, 2.0, 0.5) and hasattr(m, "refine_network")
    d = infer.build_model(infer.parse_args(base))
    assert d.ndepths == (48, 32, 8) and d.depth_interals_ratio == (4.0, 1.5, 0.75) and not hasattr(d, "refine_network")
    before = seeded_init_(CDSMVSNet(refine=False, ndepths=(48, 32, 8), depth_interals_ratio=(4.0, 1.5, 0.75)), 0)
    sd = d.state_dict()
    assert list(sd) == list(before.state_dict()) and all(torch.equal(v, sd[k]) for k, v in before.state_dict().items())


def test_new_symbols_are_declared_everywhere():
    from cds_mvsnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "cds_mvsnet_hip.h")).read()
    makefile = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "Makefile")).read()
    for name, nargs in (("cds_eval_views_u8", 14), ("cds_eval_outputs_f32", 18)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\);", header, re.M | re.S)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.load(), name)
    assert re.search(r"^SRCS\s*=.*\beval_data\.hip\b", makefile, re.M)


def test_ops_refuse_host_tensors():
    from cds_mvsnet_amd import ops
    src = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    t = (torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(4))
    with pytest.raises(ValueError):
        ops.eval_views(src, t, t)
    with pytest.raises(ValueError):
        ops.eval_outputs([torch.zeros(2, 2)] * 3, torch.zeros(3, 4, 4), torch.zeros(32, dtype=torch.int32), 4, 4)


# ---- cache -------------------------------------------------------------------------------------------------------------------------
def test_view_cache_hits_and_byte_bounded_lru():
    from cds_mvsnet_amd.eval_data import ViewCache
    loads = []

    def fetch(cache, key, nbytes=100):                         # what EvalViews does, with a stub loader
        v = cache.get(key)
        if v is None:
            v = ("view", key)
            loads.append(key)
            cache.put(key, v, nbytes)
        return v

    c = ViewCache(250)                                         # room for two views of 100 bytes
    assert fetch(c, "a") == ("view", "a") and fetch(c, "b") == ("view", "b")
    assert c.stats == {"decodes": 2, "hits": 0, "evictions": 0} and c.bytes == 200
    assert fetch(c, "a") == ("view", "a")                      # a hit; "a" is now the warm end
    assert c.stats == {"decodes": 2, "hits": 1, "evictions": 0}
    fetch(c, "c")                                              # 300 bytes > 250: the cold end, "b", goes
    assert c.keys() == ["a", "c"] and c.bytes == 200 and c.stats["evictions"] == 1
    fetch(c, "b")                                              # decoded again, "a" goes
    assert loads == ["a", "b", "c", "b"] and c.keys() == ["c", "b"]
    fetch(c, "big", 240)                                       # bytes, not entries: one large view displaces both
    assert c.keys() == ["big"] and c.bytes == 240 and c.stats["evictions"] == 4
    assert len(c) == 1 and "big" in c and "a" not in c


def test_view_cache_smaller_than_one_view_serves_then_evicts():
    from cds_mvsnet_amd.eval_data import ViewCache
    c = ViewCache(50)
    assert c.get("a") is None
    v = object()
    c.put("a", v, 100)                                         # the caller keeps `v`; the cache cannot
    assert len(c) == 0 and c.bytes == 0 and c.stats == {"decodes": 1, "hits": 0, "evictions": 1}
    assert c.get("a") is None and c.stats["hits"] == 0
    with pytest.raises(ValueError):
        ViewCache(-1)


def test_eval_views_missing_file_fails_with_its_path_before_any_device_call(tmp_path):
    from cds_mvsnet_amd.eval_data import EvalViews
    R.write_scene(str(tmp_path), "s", 3, 16, 24)
    gone = os.path.join(str(tmp_path), "s", "images", "00000002.jpg")
    os.remove(gone)
    start = threading.active_count()
    it = EvalViews(str(tmp_path), ["s"], nviews=3, max_h=16, max_w=24, device="cuda", ahead=2)     # no GPU is touched
    assert len(it) == 3
    with pytest.raises(FileNotFoundError) as e:
        next(it)
    assert gone in str(e.value)
    assert threading.active_count() == start
    with pytest.raises(StopIteration):
        next(it)
    with pytest.raises(ValueError):
        EvalViews(str(tmp_path), ["s"], nviews=3, threads=17)


# ---- writer ------------------------------------------------------------------------------------------------------------------------
def _parts(h=4, w=6):
    return [("depth", torch.arange(h * w, dtype=torch.float32).view(h, w)), ("conf3", torch.rand(h, w, 3)),
            ("img_u8", torch.randint(0, 256, (h, w, 3), dtype=torch.uint8))]


def test_output_writer_writes_packed_jobs(tmp_path):
    from cds_mvsnet_amd import mvs_io
    from cds_mvsnet_amd.eval_data import OutputWriter
    cam = np.arange(32, dtype=np.float32).reshape(2, 4, 4)
    start = threading.active_count()
    jobs = [_parts() + [(f"stage{k}", torch.full((2, 3), float(k))) for k in (1, 2, 3)] for _ in range(5)]
    with OutputWriter(str(tmp_path), depth=2) as w:            # 5 jobs through 2 buffer sets: submit waits for the writer
        for i, parts in enumerate(jobs):
            w.submit_packed("scan/{}/" + f"{i:08d}" + "{}", cam, parts)
    assert threading.active_count() == start
    for i, parts in enumerate(jobs):
        d = dict(parts)
        assert np.array_equal(mvs_io.read_pfm(str(tmp_path / "scan" / "depth_est" / f"{i:08d}.pfm"))[0], d["depth"].numpy())
        assert np.array_equal(mvs_io.read_pfm(str(tmp_path / "scan" / "confidence" / f"{i:08d}.pfm"))[0], d["conf3"].numpy())
        assert np.array_equal(mvs_io.read_pfm(str(tmp_path / "scan" / "depth_stage2" / f"{i:08d}.pfm"))[0], d["stage2"].numpy())
        assert (tmp_path / "scan" / "images" / f"{i:08d}.jpg").is_file() and (tmp_path / "scan" / "cams" / f"{i:08d}_cam.txt").is_file()
    with pytest.raises(RuntimeError):
        w.submit_packed("x/{}/0{}", cam, _parts())


def test_output_writer_error_surfaces_on_close(tmp_path):
    from cds_mvsnet_amd.eval_data import OutputWriter
    seen = []

    def failing(outdir, filename, depth, conf3, cam, img_u8, stages):
        seen.append(filename)
        raise OSError(f"disk full writing {filename}")

    cam = np.zeros((2, 4, 4), np.float32)
    start = threading.active_count()
    w = OutputWriter(str(tmp_path), depth=1, write=failing)
    w.submit_packed("a/{}/0{}", cam, _parts())
    with pytest.raises(OSError, match="disk full writing a/"):
        w.close()
    assert seen == ["a/{}/0{}"] and threading.active_count() == start
    w.close()                                                  # idempotent, the error was delivered once
    # ... or on the next submit, and the jobs after the failure are dropped without blocking
    w = OutputWriter(str(tmp_path), depth=1, write=failing)
    w.submit_packed("b/{}/0{}", cam, _parts())
    with pytest.raises(OSError, match="disk full writing b/"):
        for _ in range(3):                                     # depth 1: the second submit returns only after job one has failed
            w.submit_packed("c/{}/0{}", cam, _parts())
    w.close()
    assert threading.active_count() == start
