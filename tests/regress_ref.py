"""Float64 restatements, inputs and acceptance rules for the per-pixel kernels behind every depth map: K5 / K6 (csrc/regress.hip), the
Refinement pieces (csrc/refine.hip) and volume_normalize_ (csrc/warp.hip).  CPU torch only, nothing of the library under test.
tests/test_regress_ref_cpu.py checks this file against the goldens captured from the reference and the preconditions of the cases;
tests/test_regress_gpu.py and tests/test_refine_kernels_gpu.py compare the kernels with it.

  softargmin64 / conf_candidates      models/module.py:373-391 (depth_regression, conf_regression), models/model.py:90-92
  hypotheses64 / planes64             models/module.py:394-439 (get_cur_depth_range_samples, get_depth_range_samples) with the
                                      interpolation chain around them, models/model.py:176-193
  depth_affine64 / refine_finish64    models/module.py:351-370 with models/model.py:213-218
  deconv2d64                          the ConvTranspose2d of models/module.py:331-333

Where the CPU oracle (oracle/cds_oracle.py) takes float64 inputs unchanged (O.softargmin, O.stage_hypotheses) it IS the restatement
and is called here; what it does not return (the soft index, the un-clamped samples) is restated next to it.

Every function takes a ``dtype``: float64 is the reference, float32 is "torch's own fp32 evaluation of the same expression on the
CPU", the unit of the tests' bars.

The confidence rule.  conf = the 4-plane window sum of prob at k = clamp(trunc(sum_d p_d d)).  The index is a sum of non-negative
fp32 terms divided by another, so an implementation's index differs from the float64 one by rounding only, and where the float64
index sits within that rounding of an integer either neighbouring window is a correct answer.  conf_candidates() returns both
windows, floor(idx - eps) and floor(idx + eps); a pixel is right when it matches ONE of them.  No pixel is left out.
  eps(D) = 3 D 2^-24 max(D - 1, 1): Si = sum e_d d and Z = sum e_d are each D-term sums of non-negative numbers (relative error <= D u
  each, u = 2^-24, no cancellation), every term carries the rounding of its exp / product (<= 1 u more, counted per plane), so
  |idx_fp32 - idx| <= 3 D u idx <= 3 D u (D - 1).  (A CPU emulation of the kernel's four-slice online softmax measured at most 9e-5
  at D = 192 against this bound's 6.6e-3; the derived bound is the one used.)
"""
import torch
import torch.nn.functional as F

from oracle import cds_oracle as O

U23 = 2.0 ** -23          # one fp32 ulp of 1


# ------------------------------------------------------------------------------------------------
# K5
# ------------------------------------------------------------------------------------------------
K5_DEPTHS = (1, 2, 3, 4, 5, 7, 8, 9, 33, 48, 192, 193)
K5_SHAPES = ((1, 1), (1, 63), (3, 21), (5, 13), (8, 8), (17, 29), (40, 90))       # hw = 1, 63, 63, 65, 64, 493, 3600


def k5_pairs():
    """The (D, h, w) pairs of the K5 tests: every D at hw = 63 and hw = 65 (a wave's clamped lanes), and a covering choice of the
    rest - hw = 1 (63 clamped lanes out of 64), hw = 64 (one full workgroup), hw = 493 and 3600 (several workgroups, ragged)."""
    pairs = [(D, 1, 63) for D in K5_DEPTHS] + [(D, 5, 13) for D in K5_DEPTHS]
    pairs += [(D, 1, 1) for D in (1, 4, 193)]
    pairs += [(D, 3, 21) for D in (2, 7)]
    pairs += [(D, 8, 8) for D in (1, 3, 5, 8, 48, 192)]
    pairs += [(D, 17, 29) for D in (2, 4, 9, 33, 193)]
    pairs += [(D, 40, 90) for D in (1, 3, 7, 48, 192)]
    return pairs


K5_DIFFUSE = ("randn0.5", "randn3")                       # no planted peak: the two-candidate share is capped (test_regress_ref_cpu.py)
K5_KINDS = K5_DIFFUSE + ("randn20", "ends+30", "equal", "offset1e4", "spread90")
# the seed base is chosen so that the diffuse cases meet the two-candidate condition of test_regress_ref_cpu.py also at the shapes
# where 3 % is two pixels (a condition on the inputs alone: no kernel is involved in it)
K5_SEED = 200


def k5_logits(kind, D, h, w):
    """fp32 logits [D,h,w] of one K5 case (seeded by the case)."""
    g = torch.Generator().manual_seed(K5_SEED + 1000 * D + 10 * h + w + 7 * K5_KINDS.index(kind))
    if kind.startswith("randn"):
        return torch.randn(D, h, w, generator=g) * float(kind[5:])
    if kind == "ends+30":        # +30 on plane 0 for half the pixels, on plane D-1 for the other half: the clipped windows
        pre = torch.randn(D, h, w, generator=g) * 3.0
        first = (torch.arange(h * w).view(h, w) % 2) == 0
        pre[0][first] += 30.0
        pre[D - 1][~first] += 30.0
        return pre
    if kind == "equal":
        return torch.full((D, h, w), 0.75)
    if kind == "offset1e4":      # a common offset: only differences of logits matter
        return torch.randn(D, h, w, generator=g) * 3.0 + 1.0e4
    if kind == "spread90":       # exp underflows on most planes
        return (torch.rand(D, h, w, generator=g) * 2.0 - 1.0) * 90.0
    raise KeyError(kind)


def k5_hypotheses(D, h, w, per_pixel):
    g = torch.Generator().manual_seed(31 * D + h * w)
    planes = torch.linspace(425.0, 900.0, D) if D > 1 else torch.tensor([425.0])
    if not per_pixel:
        return planes.contiguous()
    return (planes.view(D, 1, 1) + 3.0 * torch.rand(D, h, w, generator=g)).contiguous()


def softargmin(pre, hyp, dtype=torch.float64):
    """pre [D,h,w], hyp [D] or [D,h,w] -> prob [D,h,w], depth [h,w], idx = sum_d p_d d [h,w] in ``dtype`` (module.py:373-391:
    softmax over the planes, then the expectation of the hypotheses / of the plane number)."""
    D = pre.shape[0]
    pre, hyp = pre.to(dtype), hyp.to(dtype)
    prob, depth, _ = O.softargmin(pre.unsqueeze(0), hyp.unsqueeze(0))
    idx = torch.sum(prob * torch.arange(D, dtype=dtype).view(1, D, 1, 1), dim=1)
    return prob[0], depth[0], idx[0]


def softargmin64(pre, hyp):
    return softargmin(pre, hyp, torch.float64)


def conf_eps(D):
    return 3.0 * D * 2.0 ** -24 * max(D - 1, 1)


def conf_candidates(prob64, idx64, eps):
    """The window sum p[k-1] + p[k] + p[k+1] + p[k+2] (zero outside [0, D)) at k = clamp(floor(idx - eps)) and at
    k = clamp(floor(idx + eps)): two [h,w] maps (module.py:386-390: pad (1, 2), 4-plane pool, gather at the truncated index)."""
    D = prob64.shape[0]
    padded = F.pad(prob64, (0, 0, 0, 0, 1, 2))
    win = padded[0:D] + padded[1:D + 1] + padded[2:D + 2] + padded[3:D + 3]
    out = []
    for e in (-eps, eps):
        k = torch.floor(idx64 + e).long().clamp(0, D - 1)
        out.append(torch.gather(win, 0, k.unsqueeze(0))[0])
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------
# K6
# ------------------------------------------------------------------------------------------------
# (D, H, W, scale, previous-stage divisor)
K6_CASES = ((8, 4, 4, 4, 4),          # 1x1 output from a 1x1 previous map
            (5, 4, 8, 4, 4),          # a single output row
            (32, 8, 12, 2, 4), (48, 8, 12, 1, 1),
            (2, 8, 8, 2, 2),          # even D: nl = 0, nr = 1
            (7, 36, 52, 4, 2), (8, 96, 120, 1, 4), (33, 20, 28, 2, 1))
K6_INTERVALS = (1.875, 3.75, 10.0)
K6_RANGE = (425.0, 902.5)
K6_VARIANTS = ("uniform", "at-dmin", "at-dmax")


def k6_prev(variant, D, H, W, prev_div, interval):
    """fp32 previous-stage depth [H/prev_div, W/prev_div]: uniform over the range, or within nl (nr) intervals of dmin (dmax), which
    clamps whole regions of the low (high) planes."""
    dmin, dmax = K6_RANGE
    g = torch.Generator().manual_seed(100 * D + H + W + K6_VARIANTS.index(variant))
    r = torch.rand(H // prev_div, W // prev_div, generator=g)
    nl = (D - 1) // 2
    nr = D - 1 - nl
    if variant == "uniform":
        return dmin + (dmax - dmin) * r
    if variant == "at-dmin":
        return dmin + nl * interval * r
    return dmax - nr * interval * r


def hypotheses(prev, D, interval, dmin, dmax, H, W, scale, dtype=torch.float64):
    """K6 (model.py:176-193, module.py:394-417) through the oracle in ``dtype``: prev [hp,wp] -> [D, H/scale, W/scale]."""
    t = lambda v: torch.tensor(float(v), dtype=dtype).view(1, 1, 1)   # noqa: E731
    return O.stage_hypotheses(prev.to(dtype).unsqueeze(0), D, t(interval), t(dmin), t(dmax), H, W, scale)[0]


def hypotheses64(prev, D, interval, dmin, dmax, H, W, scale):
    return hypotheses(prev, D, interval, dmin, dmax, H, W, scale, torch.float64)


def hypotheses_clamped64(prev, D, interval, dmin, dmax, H, W, scale, margin):
    """Which outputs must be EXACTLY dmin / dmax: two bool maps [D, H/scale, W/scale].  The un-clamped float64 samples
    (module.py:398-411) are restated here; an output is forced when every full-resolution sample the resize (model.py:191-193) gives
    it a non-zero weight lies beyond the limit by more than ``margin`` (an fp32 sample that far out is clamped whatever its rounding,
    and a blend of equal values with the weights 1/2, 1/2 or 1, 0 of these integer scales is that value)."""
    p = prev.double().unsqueeze(0).unsqueeze(0)
    up = F.interpolate(p, [H, W], mode="bilinear", align_corners=False)[0]                     # [1,H,W]
    nl = (D - 1) // 2
    full = (up - nl * interval) + torch.arange(D, dtype=torch.float64).view(D, 1, 1) * interval  # [D,H,W]
    maps = []
    for beyond in (full < dmin - margin, full > dmax + margin):
        share = F.interpolate(beyond.double().view(1, 1, D, H, W), [D, H // scale, W // scale], mode="trilinear", align_corners=False)
        maps.append(share[0, 0] == 1.0)
    return maps[0], maps[1]


def planes(lo, hi, D, h, w, dtype=torch.float64):
    """First-stage planes lo + k (hi - lo) / (D - 1) (module.py:425-433), [D,h,w]."""
    lo, hi = torch.tensor(float(lo), dtype=dtype), torch.tensor(float(hi), dtype=dtype)
    step = (hi - lo) / (D - 1)
    return (lo + torch.arange(D, dtype=dtype) * step).view(D, 1, 1).repeat(1, h, w)


def planes64(lo, hi, D, h, w):
    return planes(lo, hi, D, h, w, torch.float64)


# ------------------------------------------------------------------------------------------------
# Refinement pieces
# ------------------------------------------------------------------------------------------------
def _range(rng, dtype):
    """(depth_min, depth_max, interval) as the fp32 numbers the kernels read, in ``dtype``; the limits in interval units
    (model.py:214-217)."""
    r = torch.as_tensor(rng, dtype=torch.float32).to(dtype)
    return r[0] / r[2], r[1] / r[2], r[2]


def depth_affine(depth, rng, dtype=torch.float64):
    """(depth / interval - lo) / (hi - lo) * 10  (model.py:215, module.py:354-355)."""
    lo, hi, ival = _range(rng, dtype)
    return (depth.to(dtype) / ival - lo) / (hi - lo) * 10


def depth_affine64(depth, rng):
    return depth_affine(depth, rng, torch.float64)


def refine_finish(d_norm, res, rng, dtype=torch.float64):
    """((bilinear x2, align_corners=True)(d_norm [h,w]) + res [2h,2w]) / 10 * (hi - lo) + lo, times the interval
    (module.py:366-368, model.py:219)."""
    lo, hi, ival = _range(rng, dtype)
    up = F.interpolate(d_norm.to(dtype).unsqueeze(0).unsqueeze(0), scale_factor=2, mode="bilinear", align_corners=True)[0, 0]
    d = (up + res.to(dtype)) / 10
    return (d * (hi - lo) + lo) * ival


def refine_finish64(d_norm, res, rng):
    return refine_finish(d_norm, res, rng, torch.float64)


ACTIVATIONS = {"none": lambda v: v, "relu": torch.relu, "leaky01": lambda v: F.leaky_relu(v, 0.1), "sigmoid": torch.sigmoid,
               "tanh": torch.tanh}


def deconv2d(x, w, bias=None, act="none", dtype=torch.float64):
    """ConvTranspose2d k3 s2 p1 op1 (module.py:331-333) + bias + activation: x [Cin,H,W], w [Cin,Cout,3,3] -> [Cout,2H,2W]."""
    y = F.conv_transpose2d(x.to(dtype).unsqueeze(0), w.to(dtype), None if bias is None else bias.to(dtype), stride=2, padding=1,
                           output_padding=1)[0]
    return ACTIVATIONS[act](y)


def deconv2d64(x, w, bias=None, act="none"):
    return deconv2d(x, w, bias, act, torch.float64)


# ------------------------------------------------------------------------------------------------
# the bar
# ------------------------------------------------------------------------------------------------
def fp32_bar(ref64, torch32, scale=None):
    """The library's fp32-class bar for one case: 1.5 x the largest error of torch's own fp32 evaluation against float64, plus one
    fp32 ulp of the result scale (``scale``, default max |ref|).  Returns (bar, torch's error)."""
    e32 = float((torch32.double() - ref64).abs().max())
    if scale is None:
        scale = float(ref64.abs().max())
    return 1.5 * e32 + scale * U23, e32
