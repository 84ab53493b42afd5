"""The surface sampling rule of DESIGN §1.13 as mesh_sample_ref.py restates it: the counts at their exact boundaries, the
weights, the covering bound, degenerate faces and the integer colours.  No GPU: these tests pin the rule the kernels of
csrc/mesh_sample.hip are compared against in test_mesh_sample_gpu.py."""
import numpy as np

import mesh_sample_ref as R

TRI345 = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], np.float32)
F1 = np.array([[0, 1, 2]], np.int32)
GREY = np.full((3, 3), 90, np.uint8)


def test_cube():
    v, c, f = R.cube()
    out, info, n = R.sample(v, c, f, 0.5)
    assert (n == 12).all() and info == {"faces": 12, "points": 1728, "max_n": 12, "skipped": 0}
    assert out["points"].shape == (1728, 3) and out["points"].dtype == np.float32 and out["colors"].dtype == np.uint8
    assert np.array_equal(out["face"], np.repeat(np.arange(12, dtype=np.int32), 144))
    assert R.sample(v, c, f, 0.2)[1]["points"] == 10092
    # every sample lies on the cube's surface, strictly inside its face
    p = out["points"].astype(np.float64)
    on = (np.abs(p) < 1e-6) | (np.abs(p - 4) < 1e-6)
    assert (on.sum(1) == 1).all() and p.min() >= 0 and p.max() <= 4


def test_exact_boundaries_of_rule_1():
    assert R.counts(TRI345, F1, 1.0).tolist() == [5]
    assert R.counts(TRI345, F1, 0.5).tolist() == [10]
    assert R.counts(TRI345, F1, np.nextafter(1.0, 0)).tolist() == [6]
    assert R.counts(TRI345, F1, np.nextafter(1.0, 2)).tolist() == [5]
    assert R.counts(TRI345, F1, 5.0).tolist() == [1] and R.counts(TRI345, F1, 1e9).tolist() == [1]
    assert R.counts(TRI345, F1, 5.0 / R.MAX_N).tolist() == [R.MAX_N]
    assert R.counts(TRI345, F1, 1e-9).tolist() == [R.MAX_N + 1]                 # clamped: the caller refuses it
    try:
        R.sample(TRI345, GREY, F1, 1e-9)
        assert False, "no error for n > MAX_N"
    except ValueError:
        pass


def test_weights_and_centroids():
    n = 7
    k = np.arange(n * n)
    wa, wb, wc = R.weights(np.full(n * n, n), k)
    assert (wa > 0).all() and (wb > 0).all() and (wc > 0).all() and (wa + wb + wc == 3 * n).all()
    assert len({(a, b) for a, b in zip(wa.tolist(), wb.tolist())}) == n * n   # pairwise distinct centroids
    # the centroids of the lattice's sub-triangles, counted another way: upright (i, j) and inverted ones, in thirds of 1/n
    want = set()
    for r in range(n):
        for j in range(r + 1):
            want.add((3 * n - (3 * r + 2), 3 * (r - j) + 1, 3 * j + 1))
        for j in range(r):
            want.add((3 * n - (3 * r + 1), 3 * (r - j) - 1, 3 * j + 2))
    assert want == set(zip(wa.tolist(), wb.tolist(), wc.tolist()))
    # two faces over the shared edge 1-2: no sample of one equals a sample of the other, none lies on the edge
    v = np.array([[0, 0, 0], [7, 0, 0], [0, 7, 0], [7, 7, 1]], np.float32)
    f = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    out, info, cnt = R.sample(v, np.zeros((4, 3), np.uint8), f, float(np.sqrt(98.0)) / 7 * 1.0000001)
    assert cnt.tolist() == [7, 7]
    a, b = out["points"][:49], out["points"][49:]
    assert len({tuple(p) for p in a.tolist()} | {tuple(p) for p in b.tolist()}) == 98
    assert len(np.unique(a, axis=0)) == 49
    assert (np.abs(a[:, 0] + a[:, 1] - 7) > 0.1).all() and (a[:, 0] + a[:, 1] < 7).all() and (b[:, 0] + b[:, 1] > 7).all()


def test_covering():
    v, c, f = R.cube()
    rng = np.random.default_rng(0)
    for spacing in (0.5, 0.2):
        out, info, n = R.sample(v, c, f, spacing)
        face = rng.integers(0, 12, 4000)
        w = rng.dirichlet((1.0, 1.0, 1.0), 4000)
        q = (w[:, :, None] * v[f[face]].astype(np.float64)).sum(1)
        bound = 2.0 / 3.0 * spacing + 1e-5
        worst = 0.0
        for i in range(12):
            own = out["points"][out["face"] == i].astype(np.float64)
            d = np.linalg.norm(q[face == i][:, None, :] - own[None, :, :], axis=-1).min(1)
            worst = max(worst, float(d.max()))
        assert worst <= bound, (spacing, worst, bound)
        to_vertex = np.linalg.norm(q[:, None, :] - v[None].astype(np.float64), axis=-1).min(1)
        print(f"spacing {spacing}: farthest surface point {worst:.3f} from a sample (bound {bound:.3f}), {to_vertex.max():.2f} "
              "from a vertex")
        assert to_vertex.max() > 8 * bound


def test_degenerate_faces():
    v = np.array([[1, 2, 3], [1, 2, 3], [1, 2, 3], [np.nan, 0, 0], [0, 0, 0], [1, 0, 0], [0, np.inf, 0]], np.float32)
    c = np.arange(21, dtype=np.uint8).reshape(7, 3)
    f = np.array([[0, 1, 2], [3, 4, 5], [4, 5, 6], [4, 5, 4]], np.int32)
    out, info, n = R.sample(v, c, f, 0.25)
    assert n.tolist() == [1, 0, 0, 4] and info == {"faces": 4, "points": 17, "max_n": 4, "skipped": 2}
    assert out["points"][0].tolist() == [1.0, 2.0, 3.0] and out["face"].tolist() == [0] + [3] * 16
    assert np.isfinite(out["points"]).all()
    # a needle: all corners on a line, all samples on it
    a, d = np.array([1.0, -2.0, 0.5]), np.array([3.0, 4.0, 12.0])
    needle = np.stack([a, a + 13 * d / 13, a + 0.25 * d]).astype(np.float32)
    out, info, n = R.sample(needle, GREY, F1, 1.0)
    assert n.tolist() == [13] and info["points"] == 169
    rel = out["points"].astype(np.float64) - needle[0].astype(np.float64)
    t = rel @ d / (d @ d)
    assert np.abs(rel - t[:, None] * d).max() < 1e-5 and t.min() > 0 and t.max() < 1


def test_colours():
    v, c, f = R.cube()
    same = np.full((8, 3), 137, np.uint8)
    assert (R.sample(v, same, f, 0.5)[0]["colors"] == 137).all()
    # n = 1: one sample, weights 1 1 1 of 3: (2 (255) + 3) / 6 = 85.5 -> 85 in integers; two corners at 255: (2 (510) + 3) / 6 = 170
    col = np.array([[0, 0, 255], [0, 255, 255], [255, 0, 255]], np.uint8)
    out = R.sample(TRI345, col, F1, 5.0)[0]
    assert out["colors"].tolist() == [[85, 85, 255]]
    # n = 2: samples k = 0..3 have (wa, wb, wc) = (4,1,1), (1,4,1), (2,2,2), (1,1,4); channel 0 holds 255 at corner C only,
    # channel 1 at corner B only: (2 (255 w) + 6) / 12 -> w = 1: 43, w = 2: 85, w = 4: 170 (170.5 rounds half up to ... 170.5 is
    # 2046 / 12 = 170 in integers since 2 (1020) + 6 = 2046)
    wa, wb, wc = R.weights(np.full(4, 2), np.arange(4))
    assert list(zip(wa.tolist(), wb.tolist(), wc.tolist())) == [(4, 1, 1), (1, 4, 1), (2, 2, 2), (1, 1, 4)]
    out = R.sample(TRI345, col, F1, 2.5)[0]
    assert out["colors"][:, 0].tolist() == [43, 43, 85, 170] and out["colors"][:, 1].tolist() == [43, 170, 85, 43]
    assert (out["colors"][:, 2] == 255).all()
    # half up: corner colours 1, 0, 0 at n = 1 give (2 + 3) / 6 = 0; 2, 1, 0 give (6 + 3) / 6 = 1 (the mean 1.0); 1, 1, 0 give
    # (4 + 3) / 6 = 1 (the mean 0.67); 3, 0, 0 at n = 2, k = 2 (weights 2 2 2): (2 (6) + 6) / 12 = 1 (the mean 1.0)
    for cols, want in (((1, 0, 0), 0), ((2, 1, 0), 1), ((1, 1, 0), 1)):
        cc = np.array([[x] * 3 for x in cols], np.uint8)
        assert R.sample(TRI345, cc, F1, 5.0)[0]["colors"].tolist() == [[want] * 3]
