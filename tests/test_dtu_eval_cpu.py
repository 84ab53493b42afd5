"""DTU evaluation without a GPU: PLY and MAT-file readers, MATLAB rounding, the block form of MaxDistCP, the thinning
invariants of the oracle, the CLI's path resolution and its loud failures."""
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import dtu_eval_ref as R
from cds_mvsnet_amd import dtu_eval, pointcloud, synth


# ---------------------------------------------------------------------------------------------------------------- PLY
def _ply_header(fmt, n, props, extra=""):
    return (f"ply\nformat {fmt} 1.0\ncomment made by a test\nelement vertex {n}\n"
            + "".join(f"property {t} {p}\n" for t, p in props) + extra + "end_header\n").encode("ascii")


PROPS = [("double", "nx"), ("float", "y"), ("uchar", "red"), ("double", "x"), ("int", "flag"), ("float", "z")]


def _records(n, end):
    rs = np.random.RandomState(3)
    dt = np.dtype([("nx", end + "f8"), ("y", end + "f4"), ("red", "u1"), ("x", end + "f8"), ("flag", end + "i4"),
                   ("z", end + "f4")])
    rec = np.zeros(n, dt)
    for k in ("nx", "y", "x", "z"):
        rec[k] = rs.randn(n) * 100
    rec["red"], rec["flag"] = rs.randint(0, 255, n), rs.randint(-5, 5, n)
    return rec


@pytest.mark.parametrize("fmt,end", [("binary_little_endian", "<"), ("binary_big_endian", ">")])
def test_read_ply_binary_with_extra_properties_and_faces(tmp_path, fmt, end):
    rec = _records(37, end)
    faces = "element face 2\nproperty list uchar int vertex_indices\n"
    p = tmp_path / "a.ply"
    face_bytes = b"".join(struct.pack(end + "B3i", 3, 0, 1, 2) for _ in range(2))
    p.write_bytes(_ply_header(fmt, 37, PROPS, faces) + rec.tobytes() + face_bytes)
    got = pointcloud.read_ply_points(str(p))
    want = np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_read_ply_ascii_and_element_before_vertex(tmp_path):
    rec = _records(9, "<")
    lines = [" ".join(repr(float(r[k])) if k not in ("red", "flag") else str(int(r[k])) for k in rec.dtype.names) for r in rec]
    body = ("ply\nformat ascii 1.0\nelement camera 2\nproperty float f\nelement vertex 9\n"
            + "".join(f"property {t} {p}\n" for t, p in PROPS)
            + "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
            + "1.0\n2.0\n" + "\n".join(lines) + "\n3 0 1 2\n")
    p = tmp_path / "a.ply"
    p.write_text(body)
    got = pointcloud.read_ply_points(str(p))
    want = np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32)
    assert np.array_equal(got, want)


def test_read_ply_skips_binary_list_element_before_vertex(tmp_path):
    rec = _records(5, "<")
    hdr = (b"ply\nformat binary_little_endian 1.0\nelement face 2\nproperty list uchar int vertex_indices\n"
           b"element vertex 5\n" + b"".join(f"property {t} {p}\n".encode() for t, p in PROPS) + b"end_header\n")
    faces = struct.pack("<B3i", 3, 0, 1, 2) + struct.pack("<B4i", 4, 0, 1, 2, 3)
    p = tmp_path / "a.ply"
    p.write_bytes(hdr + faces + rec.tobytes())
    assert np.array_equal(pointcloud.read_ply_points(str(p)), np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32))


def test_read_ply_reads_fusion_output_and_fails_loudly(tmp_path):
    from cds_mvsnet_amd import fusion
    pts = np.random.RandomState(0).randn(13, 3).astype(np.float32)
    fusion.write_ply(str(tmp_path / "f.ply"), pts, np.zeros((13, 3), np.uint8))
    assert np.array_equal(pointcloud.read_ply_points(str(tmp_path / "f.ply")), pts)
    (tmp_path / "bad.ply").write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nend_header\n")
    with pytest.raises(ValueError, match="property y"):
        pointcloud.read_ply_points(str(tmp_path / "bad.ply"))
    (tmp_path / "no.ply").write_bytes(b"solid x\n")
    with pytest.raises(ValueError, match="not a PLY"):
        pointcloud.read_ply_points(str(tmp_path / "no.ply"))


# ------------------------------------------------------------------------------------------------------------ MAT v5
MI_INT8, MI_UINT8, MI_INT16, MI_INT32, MI_UINT32, MI_DOUBLE, MI_MATRIX, MI_COMPRESSED = 1, 2, 3, 5, 6, 9, 14, 15
MX_DOUBLE, MX_UINT8, MX_CHAR, MX_STRUCT = 6, 9, 4, 2


def _el(mtype, payload, end="<", small_ok=True):
    if small_ok and len(payload) <= 4:                      # small data element format
        return struct.pack(end + "I", (len(payload) << 16) | mtype) + payload + b"\0" * (4 - len(payload))
    return struct.pack(end + "II", mtype, len(payload)) + payload + b"\0" * ((-len(payload)) % 8)


def _matrix(name, arr, cls, store_type, store_np, end="<", logical=False, small_ok=True):
    arr = np.asarray(arr)
    flags = cls | (0x0200 if logical else 0)
    body = _el(MI_UINT32, struct.pack(end + "II", flags, 0), end, small_ok=False)
    body += _el(MI_INT32, np.asarray(arr.shape, end + "i4").tobytes(), end, small_ok=False)
    body += _el(MI_INT8, name.encode(), end, small_ok)
    body += _el(store_type, np.asarray(arr, dtype=end + store_np).ravel(order="F").tobytes(), end, small_ok)
    return struct.pack(end + "II", MI_MATRIX, len(body)) + body


def _header(end="<", version=0x0100, text=b"MATLAB 5.0 MAT-file, written by a test"):
    return text.ljust(116, b" ") + b"\0" * 8 + struct.pack(end + "H", version) + (b"IM" if end == "<" else b"MI")


def write_mat(path, variables):
    """Test-side writer of uncompressed v5 MAT-files: {name: array} (float arrays as double, bool as logical uint8)."""
    out = _header()
    for k, v in variables.items():
        v = np.asarray(v)
        if v.ndim < 2:
            v = v.reshape(1, -1) if v.ndim == 1 else v.reshape(1, 1)
        if v.dtype == bool:
            out += _matrix(k, v.astype(np.uint8), MX_UINT8, MI_UINT8, "u1", logical=True)
        else:
            out += _matrix(k, v.astype(np.float64), MX_DOUBLE, MI_DOUBLE, "f8")
    with open(path, "wb") as f:
        f.write(out)


def test_load_mat_features(tmp_path):
    rs = np.random.RandomState(1)
    nd = rs.rand(3, 4, 5) > 0.5                                    # logical, 3-d, column-major
    ints = np.array([[1.0, 2.0, 255.0], [0.0, 7.0, 9.0]])         # integral doubles stored as uint8
    neg = np.array([[-3.0], [300.0]])                             # ... as int16
    res = np.array([[0.2]])                                       # one double: not small (8 bytes)
    b = _header()
    b += _matrix("M", nd.astype(np.uint8), MX_UINT8, MI_UINT8, "u1", logical=True)
    b += _matrix("I", ints, MX_DOUBLE, MI_UINT8, "u1")
    b += _matrix("N", neg, MX_DOUBLE, MI_INT16, "i2")
    b += _matrix("Res", res, MX_DOUBLE, MI_DOUBLE, "f8")
    b += _matrix("s", np.array([[2.0]]), MX_DOUBLE, MI_UINT8, "u1")    # one byte: small-element format, padded name
    comp = zlib.compress(_matrix("BB", np.arange(6.0).reshape(2, 3), MX_DOUBLE, MI_DOUBLE, "f8"))
    b += struct.pack("<II", MI_COMPRESSED, len(comp)) + comp     # compressed elements are not padded
    b += _matrix("last", np.array([[5.0, 6.0]]), MX_DOUBLE, MI_UINT8, "u1")
    p = tmp_path / "a.mat"
    p.write_bytes(b)
    m = dtu_eval.load_mat(str(p))
    assert m["M"].dtype == bool and m["M"].shape == (3, 4, 5) and np.array_equal(m["M"], nd)
    assert m["I"].dtype == np.float64 and np.array_equal(m["I"], ints)
    assert np.array_equal(m["N"], neg) and m["N"].dtype == np.float64
    assert m["Res"][0, 0] == 0.2 and m["s"][0, 0] == 2.0
    assert np.array_equal(m["BB"], np.arange(6.0).reshape(2, 3))
    assert np.array_equal(m["last"], [[5.0, 6.0]])


def test_load_mat_big_endian_and_errors(tmp_path):
    arr = np.arange(12.0).reshape(3, 4) / 7
    p = tmp_path / "be.mat"
    p.write_bytes(_header(">") + _matrix("P", arr, MX_DOUBLE, MI_DOUBLE, "f8", end=">"))
    assert np.array_equal(dtu_eval.load_mat(str(p))["P"], arr)
    h5 = tmp_path / "v73.mat"
    h5.write_bytes(_header(version=0x0200, text=b"MATLAB 7.3 MAT-file, Platform: GLNXA64") + b"\0" * 384 + b"\x89HDF\r\n\x1a\n")
    with pytest.raises(ValueError, match="7.3"):
        dtu_eval.load_mat(str(h5))
    st = tmp_path / "st.mat"
    body = _el(MI_UINT32, struct.pack("<II", MX_STRUCT, 0), small_ok=False) + _el(MI_INT32, struct.pack("<ii", 1, 1), small_ok=False) \
        + _el(MI_INT8, b"S")
    st.write_bytes(_header() + struct.pack("<II", MI_MATRIX, len(body)) + body)
    with pytest.raises(ValueError, match="struct"):
        dtu_eval.load_mat(str(st))
    (tmp_path / "v4.mat").write_bytes(b"\0" * 200)
    with pytest.raises(ValueError):
        dtu_eval.load_mat(str(tmp_path / "v4.mat"))


def test_write_mat_roundtrip(tmp_path):
    sc = synth.make_dtu_scene(60, 40, 5.0, 8.0, 10.0)
    write_mat(str(tmp_path / "o.mat"), {"ObsMask": sc["ObsMask"], "BB": sc["BB"], "Res": sc["Res"]})
    m = dtu_eval.load_mat(str(tmp_path / "o.mat"))
    assert np.array_equal(m["ObsMask"], sc["ObsMask"]) and np.array_equal(m["BB"], sc["BB"]) and m["Res"][0, 0] == sc["Res"]


def test_load_mat_against_scipy(tmp_path):
    sio = pytest.importorskip("scipy.io")
    rs = np.random.RandomState(2)
    v = {"ObsMask": rs.rand(6, 5, 4) > 0.3, "BB": np.array([[-1.5, 2.0, 3.0], [100.0, 200.0, 300.0]]), "Res": 0.2,
         "P": np.array([[0.1], [0.2], [0.9], [-600.0]]), "I": np.array([[1.0, 2.0, 3.0]]), "i16": np.array([[-2, 5]], np.int16)}
    for compress in (False, True):
        p = str(tmp_path / f"s{int(compress)}.mat")
        sio.savemat(p, v, do_compression=compress)
        m = dtu_eval.load_mat(p)
        for k, want in v.items():
            got, want = np.asarray(m[k]), np.asarray(want)
            assert got.shape == (want.shape if want.ndim >= 2 else (1, max(want.size, 1))), (k, compress)
            assert np.array_equal(got.reshape(-1), want.reshape(-1)), (k, compress)
        assert m["ObsMask"].dtype == bool and m["i16"].dtype == np.int16


# ------------------------------------------------------------------------------------------------------------ masks
def test_matlab_round_half_away_from_zero():
    x = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, 2.4999, -3.5000001, 0.0], dtype=torch.float64)
    want = torch.tensor([1.0, 2.0, 3.0, -1.0, -2.0, -3.0, 0.0, 2.0, -4.0, 0.0], dtype=torch.float64)
    assert torch.equal(dtu_eval.matlab_round(x), want)
    assert torch.equal(torch.from_numpy(R.matlab_round(x.numpy())), want)
    assert not torch.equal(torch.round(x), want)             # why torch.round is not used


def test_masks_match_the_oracle_on_exact_half_voxels():
    sc = synth.make_dtu_scene(60, 40, 5.0, 2.0, 10.0)
    bb, res = sc["BB"], sc["Res"]
    rs = np.random.RandomState(0)
    ijk = np.stack([rs.randint(-2, s + 3, 400) for s in sc["ObsMask"].shape], 1).astype(np.float64)
    q = bb[0] + (ijk - 1.0 + rs.choice([-0.5, 0.0, 0.5, 0.25], (400, 3))) * res   # many exact .5 voxel positions
    got = dtu_eval.data_in_mask(torch.from_numpy(q), torch.from_numpy(sc["ObsMask"]), torch.from_numpy(bb), res)
    assert np.array_equal(got.numpy(), R.data_in_mask(q, sc["ObsMask"], bb, res))
    assert 0 < got.sum() < 400
    stl = torch.from_numpy(sc["stl"])
    assert np.array_equal(dtu_eval.above_plane(stl, torch.from_numpy(sc["P"])).numpy(), R.above_plane(sc["stl"], sc["P"]))


def test_distance_stats_match_the_oracle():
    d = torch.tensor([0.5, 3.0, 19.999, 20.0, 25.0, 1.0], dtype=torch.float32)
    s = dtu_eval.distance_stats(d, 20.0)
    r = R.stats(d.numpy(), 20.0)
    assert s["n"] == r["n"] == 4 and s["median"] == r["median"] == 2.0      # (1.0 + 3.0) / 2
    for k in ("mean", "median", "var"):
        assert abs(s[k] - r[k]) <= 1e-12 * abs(r[k])
    assert s["median"] == float(np.median(d.numpy()[d.numpy() < 20].astype(np.float64)))
    e = dtu_eval.distance_stats(torch.tensor([20.0, 30.0]), 20.0)
    assert e["n"] == 0 and np.isnan(e["mean"]) and np.isnan(e["median"])


# ---------------------------------------------------------------------------------------------- MaxDistCP block form
def test_block_maxdistcp_is_capped_nearest_neighbour():
    """MaxDistCP.m searches, for the from-points of a 60-block, the to-points of the block grown by 60: inside the block grid
    it finds every neighbour nearer than 60 exactly and returns >= 60 otherwise, so min(result, 60) = min(NN, 60); outside
    the grid it returns 60.  Statistics keep only values < 20, so the capped exact form gives the same statistics."""
    rs = np.random.RandomState(7)
    bb = np.array([[-37.0, 12.0, 500.0], [95.0, 130.0, 610.0]])
    cap = 60.0
    edges = [bb[0, a] + cap * np.arange(0, 4) for a in range(3)]
    def straddle(n, spread):
        pts = []
        for _ in range(n):
            pts.append([rs.choice(edges[a]) + rs.randn() * spread for a in range(3)])   # near block edges
        return np.asarray(pts)
    qto = np.concatenate([straddle(600, 8.0), rs.uniform(bb[0] - 70, bb[1] + 70, (300, 3))]).astype(np.float32)
    qfrom = np.concatenate([straddle(1200, 10.0), rs.uniform(bb[0] - 90, bb[1] + 90, (400, 3))]).astype(np.float32)
    qfrom[:5] = qto[:5]                                                      # distance 0
    block = R.max_dist_cp(qto, qfrom, bb, cap)
    brute = R.brute_nn(qfrom, qto).astype(np.float64)
    rng = np.floor((bb[1] - bb[0]) / cap)
    hi = bb[0] + (rng + 1) * cap
    inside = ((qfrom >= bb[0]) & (qfrom < hi)).all(1)
    assert inside.sum() > 200 and (~inside).sum() > 100
    assert np.array_equal(np.minimum(block[inside], cap), np.minimum(brute[inside], cap))
    assert (block[~inside] == cap).all()
    assert (brute < 20).sum() > 100 and (brute > cap).sum() > 0
    near = inside & (brute < 20)
    assert np.array_equal(block[near], brute[near])
    member = dtu_eval.in_block_grid(torch.from_numpy(qfrom), torch.from_numpy(bb), cap).numpy()
    assert np.array_equal(member, inside) and np.array_equal(member, R.block_grid_member(qfrom, bb, cap))


def test_masked_points_below_bb_are_outside_the_block_grid():
    """ObsMask's rounding admits points up to half a voxel below BB(1,:); MaxDistCP gives them 60, so they never count."""
    sc = synth.make_dtu_scene(60, 40, 1.0, 2.0, 0.5)
    bb = sc["BB"]                                           # BB(1,2) = -44.5, the STL starts near y = -40
    q = np.array([[0.0, bb[0, 1] - 0.9, 650.0], [0.0, bb[0, 1] + 0.9, 650.0], [0.0, 0.0, 650.0]])
    sc["ObsMask"][:] = True
    in_mask = R.data_in_mask(q, sc["ObsMask"], bb, sc["Res"])
    assert in_mask.tolist() == [True, True, True]
    assert dtu_eval.in_block_grid(torch.from_numpy(q), torch.from_numpy(bb), 60.0).tolist() == [False, True, True]
    d = R.max_dist_cp(sc["stl"], q.astype(np.float32), bb, 60.0)
    assert d[0] == 60.0 and d[1] < 20 and d[2] < 20


# ------------------------------------------------------------------------------------------------------- thinning
def test_oracle_thinning_invariants():
    rs = np.random.RandomState(4)
    pts = np.concatenate([rs.randn(500, 3) * 0.3, rs.uniform(-3, 3, (500, 3)), np.repeat(rs.randn(5, 3), 4, 0)]).astype(np.float32)
    order = pointcloud.thinning_order(len(pts), seed=3).numpy()
    dst = 0.2
    keep = R.reduce_pts(pts, dst, order)
    d2 = R.d2_f32(pts, pts)
    dst2 = np.float32(dst) * np.float32(dst)
    kept = np.nonzero(keep)[0]
    close = d2[np.ix_(kept, kept)] <= dst2
    np.fill_diagonal(close, False)
    assert not close.any()                                  # no two kept points within dst
    rank = np.empty(len(pts), int)
    rank[order] = np.arange(len(pts))
    for i in np.nonzero(~keep)[0]:                          # every removed point has an earlier kept point within dst
        assert (keep & (d2[i] <= dst2) & (rank < rank[i])).any()
    assert 0 < keep.sum() < len(pts)


def test_thinning_order_is_seeded_and_machine_independent():
    a = pointcloud.thinning_order(1000, seed=5)
    assert torch.equal(a, pointcloud.thinning_order(1000, seed=5))
    assert not torch.equal(a, pointcloud.thinning_order(1000, seed=6))
    assert torch.equal(torch.sort(a)[0], torch.arange(1000))
    assert a[:5].tolist() == torch.randperm(1000, generator=torch.Generator().manual_seed(5))[:5].tolist()


# ------------------------------------------------------------------------------------------------------------- CLI
def _dtu_layout(root, n, sc):
    os.makedirs(root / "Points" / "stl", exist_ok=True)
    os.makedirs(root / "ObsMask", exist_ok=True)
    from cds_mvsnet_amd import fusion
    fusion.write_ply(str(root / "Points" / "stl" / f"stl{n:03d}_total.ply"), sc["stl"], np.zeros_like(sc["stl"], np.uint8))
    write_mat(str(root / "ObsMask" / f"ObsMask{n}_10.mat"), {"ObsMask": sc["ObsMask"], "BB": sc["BB"], "Res": sc["Res"]})
    write_mat(str(root / "ObsMask" / f"Plane{n}.mat"), {"P": sc["P"].reshape(4, 1)})


def test_cli_path_resolution_and_loud_failures(tmp_path):
    assert dtu_eval.scan_number("scan9") == 9 and dtu_eval.scan_number("9") == 9 and dtu_eval.scan_number("scan114") == 114
    paths = dtu_eval.dtu_scan_paths("/d", 9)
    assert paths["stl"] == os.path.join("/d", "Points", "stl", "stl009_total.ply")
    assert paths["obsmask"] == os.path.join("/d", "ObsMask", "ObsMask9_10.mat")
    assert paths["plane"] == os.path.join("/d", "ObsMask", "Plane9.mat")
    (tmp_path / "list.txt").write_text("scan1\nscan9\n\n")
    assert dtu_eval.scan_names(str(tmp_path / "list.txt"), None) == ["scan1", "scan9"]
    assert dtu_eval.scan_names(None, "1, 4,scan9") == ["scan1", "scan4", "scan9"]
    with pytest.raises(ValueError):
        dtu_eval.scan_number("scanX")

    sc = synth.make_dtu_scene(60, 40, 5.0, 8.0, 10.0)
    data = tmp_path / "MVS Data"
    _dtu_layout(data, 9, sc)
    gt = dtu_eval.load_dtu_scan(str(data), 9)
    assert np.array_equal(gt["stl"], sc["stl"]) and np.array_equal(gt["ObsMask"], sc["ObsMask"])
    assert np.array_equal(gt["BB"], sc["BB"]) and gt["Res"] == sc["Res"] and np.array_equal(gt["P"], sc["P"])
    plydir = tmp_path / "out"
    os.makedirs(plydir)
    with pytest.raises(FileNotFoundError, match="scan9.ply"):          # the fused cloud is missing
        dtu_eval.main(["--datapath", str(data), "--plydir", str(plydir), "--scans", "9"])
    for k in (9, 4):
        (plydir / f"scan{k}.ply").write_bytes((tmp_path / "MVS Data" / "Points" / "stl" / "stl009_total.ply").read_bytes())
    with pytest.raises(FileNotFoundError, match="stl004_total.ply"):   # ground truth of scan 4 is missing
        dtu_eval.main(["--datapath", str(data), "--plydir", str(plydir), "--scans", "9,4"])
    os.remove(data / "ObsMask" / "Plane9.mat")
    with pytest.raises(FileNotFoundError, match="Plane9.mat"):
        dtu_eval.main(["--datapath", str(data), "--plydir", str(plydir), "--scans", "9"])
    with pytest.raises(FileNotFoundError, match="Plane9.mat"):
        dtu_eval.load_dtu_scan(str(data), 9)


def test_cpu_tensors_fail_loudly():
    pts = torch.rand(10, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointcloud.nearest_distance(pts, pts, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointcloud.reduce_points(pts, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dtu_eval.evaluate(pts, {"stl": np.zeros((3, 3), np.float32)})
    with pytest.raises(SystemExit):
        dtu_eval.main(["--datapath", "x", "--plydir", "y", "--scans", "1", "--device", "cpu"])
