"""tests/regress_ref.py against the goldens captured from the reference (tests/golden/make_golden.py: g3_regress_*, g4_hypotheses),
against the CPU oracle, and the preconditions of the GPU cases.  No GPU.

The goldens are the reference's fp32 results, the restatements are float64, so they agree to fp32 rounding only.  The bounds below
are forward bounds of that rounding (u = 2^-24, worst case, every rounding in the same direction); the measured differences are
printed (``pytest -s``) and sit one to three orders below them:

  prob      (D + 4) u             Z is a D-term sum of non-negative terms (<= D u relative), exp, the subtraction of the maximum and
                                  the division add <= 4 u to a value <= 1
  depth     2 (D + 4) u max|hyp|  the prob error over D planes, and the D-term sum of the products
  conf      4 x the prob bound    four planes; EVERY golden pixel must match one of the two candidate windows (regress_ref.py)
  K6        24 x 2^-15            <= 24 roundings on the way (two resizes of 9 each, the sample and the two clamps), each half an ulp of
                                  a value < 1024
  planes    (D + 2) x 2^-15       the step's rounding reaches plane k k-fold; the product and the sum
"""
import pytest
import torch

import regress_ref as R
from conftest import load_golden
from oracle import cds_oracle as O

U = 2.0 ** -24


@pytest.mark.parametrize("tag", ["d48", "d8", "d192"])
def test_softargmin64_reproduces_golden(tag):
    g = load_golden(f"g3_regress_{tag}")
    D = g["prob_pre"].shape[0]
    prob, depth, idx = R.softargmin64(g["prob_pre"], g["hyp"])
    assert prob.dtype == depth.dtype == idx.dtype == torch.float64
    e_p = float((prob - g["prob"]).abs().max())
    e_d = float((depth - g["depth"]).abs().max())
    c0, c1 = R.conf_candidates(prob, idx, R.conf_eps(D))
    e_c = torch.minimum((c0 - g["conf"]).abs(), (c1 - g["conf"]).abs())
    print(f"g3_regress_{tag}: |golden - float64| prob {e_p:.2e} (bound {(D + 4) * U:.2e}), depth {e_d:.2e} "
          f"(bound {2 * (D + 4) * U * float(g['hyp'].abs().max()):.2e}), conf vs the nearer candidate {float(e_c.max()):.2e}, "
          f"pixels with two candidates {float((c0 != c1).double().mean()):.4f}")
    assert e_p <= (D + 4) * U
    assert e_d <= 2 * (D + 4) * U * float(g["hyp"].abs().max())
    assert bool((e_c <= 4 * (D + 4) * U).all())
    # the float32 evaluation of the same restatement is the reference's own arithmetic, up to the host's vectorised exp and sum
    p32, d32, _ = R.softargmin(g["prob_pre"], g["hyp"], torch.float32)
    assert p32.dtype == d32.dtype == torch.float32
    assert float((p32 - g["prob"]).abs().max()) <= (D + 4) * U
    assert float((d32 - g["depth"]).abs().max()) <= 2 * (D + 4) * U * float(g["hyp"].abs().max())


def test_conf_candidates_window_and_clamp():
    """The window is p[k-1..k+2] with zeros outside, the index is clamped: hand-made one-hot volumes."""
    D = 5
    for peak, want in ((0, 1.0), (D - 1, 1.0), (2, 1.0)):
        prob = torch.zeros(D, 1, 1, dtype=torch.float64)
        prob[peak] = 1.0
        idx = torch.full((1, 1), float(peak), dtype=torch.float64)
        lo, hi = R.conf_candidates(prob, idx, 1e-3)
        # floor(peak - eps) = peak - 1: the window [peak-2, peak+1] still holds the peak; so does [peak-1, peak+2]
        assert float(lo) == want and float(hi) == want
    prob = torch.tensor([0.1, 0.2, 0.3, 0.25, 0.15], dtype=torch.float64).view(D, 1, 1)
    lo, hi = R.conf_candidates(prob, torch.full((1, 1), 1.0), 1e-3)       # k = 0: p0+p1+p2, k = 1: p0+p1+p2+p3
    assert abs(float(lo) - 0.6) < 1e-15 and abs(float(hi) - 0.85) < 1e-15
    lo, hi = R.conf_candidates(prob, torch.full((1, 1), 3.9999), 1e-3)    # k = 3: p2+p3+p4, k = 4: p3+p4
    assert abs(float(lo) - 0.7) < 1e-15 and abs(float(hi) - 0.4) < 1e-15
    lo, hi = R.conf_candidates(prob, torch.full((1, 1), 2.5), 1e-3)       # away from an integer: one window
    assert float(lo) == float(hi) and abs(float(lo) - 0.9) < 1e-15


def test_hypotheses64_reproduces_golden():
    g = load_golden("g4_hypotheses")
    dv = g["depth_values"]
    H, W = int(g["H"]), int(g["W"])
    dmin, dmax, dint = float(dv[0, 0]), float(dv[0, -1]), float(dv[0, 1] - dv[0, 0])
    s1 = R.planes64(dmin, dmax, 48, H // 4, W // 4)
    e = float((s1 - g["s1"][0]).abs().max())
    print(f"g4 s1: |golden - float64| {e:.2e} (bound {50 * 2.0 ** -15:.2e})")
    assert e <= 50 * 2.0 ** -15
    assert torch.equal(R.planes(dmin, dmax, 48, H // 4, W // 4, torch.float32), g["s1"][0])
    for tag in ("s2", "s3", "s2x4"):
        D, ratio, scale = g[tag + "_meta"]
        D, scale = int(D), int(scale)
        interval = float(torch.tensor(float(ratio)) * (dv[0, 1] - dv[0, 0]))          # the fp32 product the reference forms
        prev = g[tag + "_prev"][0]
        out = R.hypotheses64(prev, D, interval, dmin, dmax, H, W, scale)
        e = float((out - g[tag][0]).abs().max())
        print(f"g4 {tag}: |golden - float64| {e:.2e} (bound {24 * 2.0 ** -15:.2e})")
        assert out.dtype == torch.float64 and e <= 24 * 2.0 ** -15, tag
        o32 = R.hypotheses(prev, D, interval, dmin, dmax, H, W, scale, torch.float32)
        assert o32.dtype == torch.float32 and float((o32 - g[tag][0]).abs().max()) <= 24 * 2.0 ** -15, tag
        # the forced-clamp maps: where they hold, float64 and the golden are exactly the limit; the golden clamps on both sides
        lo, hi = R.hypotheses_clamped64(prev, D, interval, dmin, dmax, H, W, scale, dmax * 2.0 ** -22)
        assert tag == "s3" or (lo.any() and hi.any()), tag          # (s3's 8 narrow planes never reach a limit)
        assert bool((out[lo] == dmin).all()) and bool((out[hi] == dmax).all()), tag
        assert bool((g[tag][0][lo] == dmin).all()) and bool((g[tag][0][hi] == dmax).all()), tag
    assert dint > 0


def test_refinement_scaling_matches_oracle(seeded_state):
    """refine_finish64 o depth_affine64 = O.refinement with a zero residual (module.py:354-355, 366-368), and the interval form
    (model.py:213-219) = the same network on depth / interval, times the interval."""
    sd = {k: v.double() for k, v in seeded_state(True).state_dict().items()}
    sd["refine_network.res.weight"] = torch.zeros_like(sd["refine_network.res.weight"])
    g = torch.Generator().manual_seed(2)
    h, w = 7, 10
    depth0 = (170.3 + 191.6 * torch.rand(h, w, generator=g))
    img = torch.rand(1, 3, 2 * h, 2 * w, generator=g).double()
    zero = torch.zeros(2 * h, 2 * w)
    for ival in (1.0, 2.5, 0.37):
        rng = torch.tensor([170.3, 361.9, ival])                                    # fp32, as the kernels read it
        r64 = rng.double()
        want = O.refinement(img, (depth0.double() / r64[2]).view(1, 1, h, w), (r64[0] / r64[2]).view(1), (r64[1] / r64[2]).view(1),
                            sd)[0, 0] * r64[2]
        d = R.depth_affine64(depth0, rng)
        got = R.refine_finish64(d, zero, rng)
        assert d.dtype == got.dtype == torch.float64
        assert float(d.min()) >= -1e-9 and float(d.max()) <= 10.0 + 1e-9
        assert float((got - want).abs().max()) <= 1e-12 * 361.9, ival
        # corners of an align_corners=True resize are the input's corners: the round trip returns the depth
        for (y, x), (Y, X) in (((0, 0), (0, 0)), ((0, w - 1), (0, 2 * w - 1)), ((h - 1, 0), (2 * h - 1, 0)),
                               ((h - 1, w - 1), (2 * h - 1, 2 * w - 1))):
            assert abs(float(got[Y, X]) - float(depth0[y, x])) <= 1e-12 * 361.9


def test_deconv2d64_is_the_scatter_definition():
    """out[co][2y-1+ky][2x-1+kx] += x[ci][y][x] w[ci][co][ky][kx] (stride 2, pad 1, output_padding 1), written out as loops."""
    g = torch.Generator().manual_seed(9)
    Cin, Cout, H, W = 2, 3, 3, 4
    x = torch.randn(Cin, H, W, generator=g, dtype=torch.float64)
    wt = torch.randn(Cin, Cout, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    want = b.view(Cout, 1, 1).repeat(1, 2 * H, 2 * W)
    for ci in range(Cin):
        for y in range(H):
            for xx in range(W):
                for ky in range(3):
                    for kx in range(3):
                        Y, X = 2 * y - 1 + ky, 2 * xx - 1 + kx
                        if 0 <= Y < 2 * H and 0 <= X < 2 * W:
                            want[:, Y, X] += x[ci, y, xx] * wt[ci, :, ky, kx]
    assert float((R.deconv2d64(x, wt, b) - want).abs().max()) < 1e-13
    assert torch.equal(R.deconv2d64(x, wt, b, "relu"), torch.relu(R.deconv2d64(x, wt, b)))


@pytest.mark.parametrize("D,h,w", R.k5_pairs())
def test_k5_diffuse_inputs_have_few_two_candidate_pixels(D, h, w):
    """CONDITION on the inputs (not a measurement of any kernel): on the diffuse cases at most 3 % of the pixels may sit within
    eps(D) of an integer index, i.e. have two acceptable confidence windows; everywhere else the confidence test pins one window.
    (The peaked and constant cases are exempt: their index is an integer by construction and both windows are still checked.)"""
    for kind in R.K5_DIFFUSE:
        pre = R.k5_logits(kind, D, h, w)
        prob, _, idx = R.softargmin64(pre, R.k5_hypotheses(D, h, w, False))
        c0, c1 = R.conf_candidates(prob, idx, R.conf_eps(D))
        share = float((c0 != c1).double().mean())
        assert share <= 0.03, (kind, share)


def test_k5_pairs_cover_the_issue():
    pairs = R.k5_pairs()
    assert len(set(pairs)) == len(pairs) and 35 <= len(pairs) <= 50
    for hw in (63, 65):
        assert {D for D, h, w in pairs if h * w == hw} >= set(R.K5_DEPTHS)
    assert {h * w for _, h, w in pairs} >= {1, 63, 64, 65, 493, 3600}
    assert {(h, w) for _, h, w in pairs} == set(R.K5_SHAPES)
    for D, h, w in pairs:                  # the planted case really peaks at both ends, the spread case really underflows
        pre = R.k5_logits("ends+30", D, h, w)
        assert pre.dtype == torch.float32
        if h * w > 1 and D > 1:
            am = pre.argmax(0).flatten()
            assert bool((am[0::2] == 0).all()) and bool((am[1::2] == D - 1).all())
    p64 = torch.softmax(R.k5_logits("spread90", 192, 8, 8).double(), 0)
    assert float((p64 < 2.0 ** -126).float().mean()) > 0.5          # below the smallest normal fp32 number on most planes


@pytest.mark.parametrize("case", R.K6_CASES)
def test_k6_clamp_variants_clamp_regions(case):
    """CONDITION on the inputs: the two clamp variants force outputs to the limits (so the exactness assertion of the GPU test is
    not empty), and the forced outputs of the float64 reference are exactly the limits."""
    D, H, W, scale, div = case
    dmin, dmax = R.K6_RANGE
    for interval in R.K6_INTERVALS:
        for variant in R.K6_VARIANTS:
            prev = R.k6_prev(variant, D, H, W, div, interval)
            assert prev.dtype == torch.float32 and prev.shape == (H // div, W // div)
            assert float(prev.min()) >= dmin and float(prev.max()) <= dmax
            out = R.hypotheses64(prev, D, interval, dmin, dmax, H, W, scale)
            assert out.shape == (D, H // scale, W // scale)
            lo, hi = R.hypotheses_clamped64(prev, D, interval, dmin, dmax, H, W, scale, dmax * 2.0 ** -22)
            assert bool((out[lo] == dmin).all()) and bool((out[hi] == dmax).all())
            if variant == "at-dmin" and D > 2:
                assert lo[0].float().mean() > 0.5            # the first plane: first = prev - nl interval <= dmin everywhere
            if variant == "at-dmax":
                assert hi[D - 1].float().mean() > 0.5
