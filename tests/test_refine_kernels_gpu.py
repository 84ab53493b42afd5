"""The Refinement kernels of csrc/refine.hip on their own - ops.deconv2d_k3s2, ops.depth_affine, ops.refine_finish - against the float64
restatements of tests/regress_ref.py (models/module.py:331-333, 351-370 with models/model.py:213-219), at the shapes where they take
another path: 1-pixel, 1-row and 1-column inputs (the deconvolution's right / bottom guards, the sy = 0 / sx = 0 branches of the x2
resize), no bias, every activation code, a caller-supplied output buffer, a depth interval other than 1 read from a device block.

Bar (regress_ref.fp32_bar): max |kernel - float64| <= 1.5 x max |torch fp32 on the CPU - float64| + one fp32 ulp of the output scale,
per case.  No bar comes from a kernel's output.

Measured on an MI355X: the case nearest its bar per row, and the largest kernel error / torch-fp32 error over the cases where torch's
own error is at least the ulp term:

  kernel             worst err / bar   (that case: kernel, torch fp32, bar)                            worst err / torch
  deconv2d_k3s2      0.75              Cin=8 1x1 bias, tanh:           1.35e-07, 4.02e-08, 1.79e-07     1.46
  depth_affine       0.49              32x48 (425, 905, 0.37):         2.23e-06, 2.23e-06, 4.53e-06     1.00
  refine_finish      0.67              32x48 (425, 905, 2.5):          9.46e-04, 8.66e-04, 1.41e-03     1.09

With one fmaf chain over all taps of an output the deconvolution missed this bar at Cin = 32 (4.64e-06 against a bar of 3.88e-06 at
9x13: a 128-term chain at the odd-odd outputs, twice torch's error).  The kernel now sums the taps of one input channel first and adds
that to the accumulator, a Cin-term chain: 2.12e-06 in the same case (about 5 % more time in this kernel).  refine_finish's
error on a rough map is the fp32 rounding of the sample position, which torch shares.
"""
import math

import pytest
import torch

import regress_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cds_mvsnet_amd import ops as o
    return o


def _acts():
    from cds_mvsnet_amd import _lib
    return {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "leaky01": _lib.ACT_LEAKY01, "sigmoid": _lib.ACT_SIGMOID,
            "tanh": _lib.ACT_TANH}                     # every code cds_apply_act implements


def _ratio(err, e32):
    return err / e32 if e32 > 0 else 0.0


def _ulp32(x):
    """The spacing of fp32 numbers at |x| (float64 tensor)."""
    return torch.pow(2.0, torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)


# ------------------------------------------------------------------------------------------------
# deconv2d_k3s2
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (6, 1), (9, 13), (16, 24)])
@pytest.mark.parametrize("Cin", [1, 8, 32])
def test_deconv2d_k3s2_vs_float64(Cin, H, W, ops):
    from cds_mvsnet_amd.model import _pack_deconv2d
    g = torch.Generator().manual_seed(100 * Cin + 10 * H + W)
    x = torch.randn(Cin, H, W, generator=g)
    wt = torch.randn(Cin, 8, 3, 3, generator=g) * 0.3
    b = torch.randn(8, generator=g)
    x_d, w_d, b_d = x.to(DEV), _pack_deconv2d(wt).to(DEV), b.to(DEV)
    worst = (0.0, 0.0)
    for bias, bias_d in ((b, b_d), (None, None)):
        for name, code in _acts().items():
            ref = R.deconv2d64(x, wt, bias, name)
            bar, e32 = R.fp32_bar(ref, R.deconv2d(x, wt, bias, name, torch.float32))
            out = ops.deconv2d_k3s2(x_d, w_d, bias_d, code)
            assert out.shape == (8, 2 * H, 2 * W)
            cat = torch.full((16, 2 * H, 2 * W), -77.0, device=DEV)               # the model's form: the first half of a concat buffer
            ret = ops.deconv2d_k3s2(x_d, w_d, bias_d, code, out=cat[:8])
            tag = (bias is not None, name)
            assert ret.data_ptr() == cat.data_ptr() and torch.equal(cat[:8], out), tag
            assert bool((cat[8:] == -77.0).all()), tag
            err = float((out.cpu().double() - ref).abs().max())
            worst = (max(worst[0], err / bar), max(worst[1], _ratio(err, e32)))
            print(f"deconv Cin={Cin} {H}x{W} bias={tag[0]} {name}: {err:.2e} (torch {e32:.2e}, bar {bar:.2e})")
            assert err <= bar, (tag, err, bar)
    print("RATIO DECONV Cin=%d %dx%d deconv=%.3f/%.3f" % (Cin, H, W, worst[0], worst[1]))


@pytest.mark.parametrize("H,W", [(1, 1), (6, 1), (9, 13)])
def test_deconv2d_k3s2_integers_exact(H, W, ops):
    """Small integers: every product and partial sum is an integer below 2^24, so any summation order gives the float64 result."""
    from cds_mvsnet_amd import _lib
    from cds_mvsnet_amd.model import _pack_deconv2d
    g = torch.Generator().manual_seed(H * W)
    x = torch.randint(-3, 4, (8, H, W), generator=g).float()
    wt = torch.randint(-2, 3, (8, 8, 3, 3), generator=g).float()
    b = torch.randint(-5, 6, (8,), generator=g).float()
    for name, code in (("none", _lib.ACT_NONE), ("relu", _lib.ACT_RELU)):
        out = ops.deconv2d_k3s2(x.to(DEV), _pack_deconv2d(wt).to(DEV), b.to(DEV), code).cpu()
        assert torch.equal(out.double(), R.deconv2d64(x, wt, b, name)), name


# ------------------------------------------------------------------------------------------------
# depth_affine, refine_finish
# ------------------------------------------------------------------------------------------------
def _ranges():
    """(depth_min, depth_max, interval): as Python floats (interval 1) and as the 3-element device tensor of a geometry block."""
    out = [("floats", (425.0, 905.0, 1.0))]
    for lo, hi in ((425.0, 905.0), (170.3, 361.9)):
        for ival in (1.0, 2.5, 0.37):
            out.append(("device", (lo, hi, ival)))
    return out


def _call_range(form, rng):
    """The (lo, hi) arguments of ops.depth_affine / ops.refine_finish for one range."""
    if form == "floats":
        return rng[0], rng[1]
    return torch.tensor(rng, dtype=torch.float32).to(DEV), None


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (7, 1), (19, 27), (32, 48)])
def test_depth_affine_and_refine_finish_vs_float64(h, w, ops):
    g = torch.Generator().manual_seed(h * 100 + w)
    worst_a, worst_f = (0.0, 0.0), (0.0, 0.0)
    for form, rng in _ranges():
        lo, hi, _ = torch.tensor(rng, dtype=torch.float32).tolist()
        depth = (lo + (hi - lo) * torch.rand(h, w, generator=g)).clamp(lo, hi)
        d_norm = 10.0 * torch.rand(h, w, generator=g)
        res = 0.3 * torch.randn(2 * h, 2 * w, generator=g)
        a, b = _call_range(form, rng)
        # depth_affine
        ref = R.depth_affine64(depth, rng)
        bar, e32 = R.fp32_bar(ref, R.depth_affine(depth, rng, torch.float32), scale=10.0)
        got = ops.depth_affine(depth.to(DEV), a, b)
        err = float((got.cpu().double() - ref).abs().max())
        worst_a = (max(worst_a[0], err / bar), max(worst_a[1], _ratio(err, e32)))
        print(f"affine {h}x{w} {form} {rng}: {err:.2e} (torch {e32:.2e}, bar {bar:.2e})")
        assert got.shape == (h, w) and err <= bar, (form, rng, err, bar)
        # refine_finish on an independent rough map
        ref = R.refine_finish64(d_norm, res, rng)
        bar, e32 = R.fp32_bar(ref, R.refine_finish(d_norm, res, rng, torch.float32))
        got = ops.refine_finish(d_norm.to(DEV), res.to(DEV), a, b)
        err = float((got.cpu().double() - ref).abs().max())
        worst_f = (max(worst_f[0], err / bar), max(worst_f[1], _ratio(err, e32)))
        print(f"finish {h}x{w} {form} {rng}: {err:.2e} (torch {e32:.2e}, bar {bar:.2e})")
        assert got.shape == (2 * h, 2 * w) and err <= bar, (form, rng, err, bar)
        if form == "floats":       # the float form is the device form with interval 1
            dev3 = torch.tensor(rng, dtype=torch.float32).to(DEV)
            assert torch.equal(got, ops.refine_finish(d_norm.to(DEV), res.to(DEV), dev3))
            assert torch.equal(ops.depth_affine(depth.to(DEV), a, b), ops.depth_affine(depth.to(DEV), dev3))
    print("RATIO REFINE %dx%d affine=%.3f/%.3f finish=%.3f/%.3f" % (h, w, *worst_a, *worst_f))


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (7, 1), (19, 27), (32, 48)])
def test_refine_finish_constant_map(h, w, ops):
    """res = 0 on a constant map returns the un-normalised constant within 2 ulp.  Limits 425 / 905 and interval 1 are exact, so the
    roundings are: two blends of equal values (<= 4 x 2^-24 relative), the division by 10, the product with 480 (<= 6 x 2^-24 of 177.6
    in all = 6.4e-5) and the sum (half an ulp of 602.6 = 3.1e-5): 9.4e-5 in the worst case, 2 ulp = 1.2e-4."""
    c = torch.tensor(3.7)
    want = float(c.double() / 10 * 480.0 + 425.0)
    got = ops.refine_finish(torch.full((h, w), float(c), device=DEV), torch.zeros(2 * h, 2 * w, device=DEV), 425.0, 905.0).cpu()
    err = float((got.double() - want).abs().max())
    assert err <= 2 * 2.0 ** (math.floor(math.log2(want)) - 23), err


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (7, 1), (19, 27), (32, 48)])
def test_refine_round_trip_at_grid_points(h, w, ops):
    """refine_finish(depth_affine(d), 0) returns d within 4 ulp where the x2 align_corners resize samples an input pixel exactly: output
    (Y, X) reads input Y (h - 1) / (2h - 1), an integer only at Y = 0 and Y = 2h - 1 (h - 1 and 2h - 1 are coprime) - the four corners,
    whole columns / rows when h = 1 / w = 1.  The map is smooth (a ramp of at most a tenth of the range per pixel), so that the fp32
    rounding of the sample POSITION at the far corner (<= (h - 1) 2^-24 pixels, the same in torch) stays far below an ulp."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    ramp = 0.15 + 0.7 * (ys / max(h, 10) + xs / max(w, 10)) / 2 + 0.02 * torch.sin(ys + 2 * xs)
    rows = [0] if h == 1 else [0, h - 1]
    cols = [0] if w == 1 else [0, w - 1]
    for form, rng in _ranges():
        lo, hi, _ = torch.tensor(rng, dtype=torch.float32).tolist()
        d = (lo + (hi - lo) * ramp).contiguous()
        a, b = _call_range(form, rng)
        back = ops.refine_finish(ops.depth_affine(d.to(DEV), a, b), torch.zeros(2 * h, 2 * w, device=DEV), a, b).cpu().double()
        for y in rows:
            for x in cols:
                Y = slice(None) if h == 1 else (0 if y == 0 else 2 * h - 1)
                X = slice(None) if w == 1 else (0 if x == 0 else 2 * w - 1)
                want = d[y, x].double()
                err = (back[Y, X] - want).abs().max()
                assert float(err) <= 4 * float(_ulp32(want)), (form, rng, y, x, float(err))
