"""K5 (cds_softargmin_conf_f32), K6 (cds_depth_hypotheses_f32, cds_depth_planes_f32), the soft-argmin backward and volume_normalize_
against the float64 restatements of tests/regress_ref.py, at the shapes where these kernels take another path: hw below / at / over a
wave's 64 pixels (clamped lanes keep K5's shuffles alive), D < 4 (depth slices without planes), D % 4 and D % 8 != 0 (clamped plane
loads), 1-wide previous maps and 1-row outputs, even D, ranges clamped over whole regions.

Bar (regress_ref.fp32_bar): max |kernel - float64| <= 1.5 x max |torch fp32 on the CPU - float64| + one fp32 ulp of the result scale,
per case.  The confidence is held, at EVERY pixel, to 4 x the case's prob bar of one of the two candidate windows of that pixel
(regress_ref.conf_candidates; tests/test_regress_ref_cpu.py caps how many pixels have two).  No bar comes from a kernel's output.

Measured on an MI355X: the case nearest its bar per row, and the largest kernel error / torch-fp32 error over the cases where torch's
own error is at least the ulp term (elsewhere the quotient says nothing: torch is exact at D = 1, say):

  kernel                         worst err / bar   (that case: kernel, torch fp32, bar)                        worst err / torch
  K5 prob                        0.63              D=7 1x63 spread90:     1.46e-07, 7.51e-08, 2.32e-07          1.20
  K5 depth                       0.96              D=192 1x63 randn20:    2.89e-04, 1.29e-04, 3.00e-04          2.24
  K5 conf (nearer candidate)     0.17              D=4 5x13 randn0.5:     1.19e-07, -, 6.89e-07                 -
  K6 hypotheses                  0.46              D=7 36x52 /4 at-dmax:  9.16e-05, 6.10e-05, 1.99e-04          1.00
  K6 planes                      bit-equal to torch fp32
  volume_normalize_              0.78 of 1 ulp (planar and channels-last)

K5's depth sits above 1.5 x torch at D = 192 (a 48-term sequential sum per slice against torch's blocked sum) and passes on the ulp
term of the bar; everything else is inside 1.5 x on its own.
"""
import pytest
import torch
import torch.nn.functional as F

import regress_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cds_mvsnet_amd import ops as o
    return o


def _ratio(err, e32):
    return err / e32 if e32 > 0 else 0.0


def _close(got, ref, name, rel):
    """max |got - ref| <= rel x max |ref| (the measure of tests/test_train2d_gpu.py)."""
    ref, got = ref.detach().double().cpu(), got.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    assert err <= rel * scale, f"{name}: max abs err {err:.3e} vs scale {scale:.3e}"


# ------------------------------------------------------------------------------------------------
# K5
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,h,w", R.k5_pairs())
def test_k5_vs_float64(D, h, w, ops):
    worst = {"prob": (0.0, 0.0), "depth": (0.0, 0.0), "conf": (0.0, 0.0)}
    for kind in R.K5_KINDS:
        pre = R.k5_logits(kind, D, h, w)
        pre_d = pre.to(DEV)
        for per_pixel in (True, False):
            hyp = R.k5_hypotheses(D, h, w, per_pixel)
            p64, d64, i64 = R.softargmin64(pre, hyp)
            p32, d32, _ = R.softargmin(pre, hyp, torch.float32)
            bar_p, e32_p = R.fp32_bar(p64, p32, scale=1.0)
            bar_d, e32_d = R.fp32_bar(d64, d32)
            depth, conf, prob = ops.softargmin_conf(pre_d, hyp.to(DEV), want_prob=True)
            depth2, conf2 = ops.softargmin_conf(pre_d, hyp.to(DEV))                         # prob == nullptr
            depth3, conf3, prob3 = ops.softargmin_conf(pre_d, hyp.to(DEV), want_prob=True)  # a second run
            tag = (kind, per_pixel)
            assert torch.equal(depth, depth2) and torch.equal(conf, conf2), tag
            assert torch.equal(depth, depth3) and torch.equal(conf, conf3) and torch.equal(prob, prob3), tag
            if not per_pixel:     # [D] planes == the same planes broadcast per pixel
                bc = hyp.view(D, 1, 1).expand(D, h, w).contiguous().to(DEV)
                depth4, conf4, prob4 = ops.softargmin_conf(pre_d, bc, want_prob=True)
                assert torch.equal(depth, depth4) and torch.equal(conf, conf4) and torch.equal(prob, prob4), tag
            e_p = float((prob.cpu().double() - p64).abs().max())
            e_d = float((depth.cpu().double() - d64).abs().max())
            c0, c1 = R.conf_candidates(p64, i64, R.conf_eps(D))
            c = conf.cpu().double()
            e_c = torch.minimum((c - c0).abs(), (c - c1).abs())
            for name, err, bar, e32 in (("prob", e_p, bar_p, e32_p), ("depth", e_d, bar_d, e32_d),
                                        ("conf", float(e_c.max()), 4 * bar_p, 4 * e32_p)):
                worst[name] = (max(worst[name][0], err / bar), max(worst[name][1], _ratio(err, e32)))
            print(f"K5 D={D} {h}x{w} {kind} pp={int(per_pixel)}: prob {e_p:.2e} (torch {e32_p:.2e}, bar {bar_p:.2e}) "
                  f"depth {e_d:.2e} (torch {e32_d:.2e}, bar {bar_d:.2e}) conf {float(e_c.max()):.2e} (bar {4 * bar_p:.2e})")
            assert e_p <= bar_p, (tag, e_p, bar_p)
            assert e_d <= bar_d, (tag, e_d, bar_d)
            assert bool((e_c <= 4 * bar_p).all()), (tag, float(e_c.max()), 4 * bar_p)        # every pixel
    print("RATIO K5 D=%d %dx%d " % (D, h, w) + " ".join(f"{k}={v[0]:.3f}/{v[1]:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("D", [1, 3, 5, 33])
@pytest.mark.parametrize("h,w", [(1, 63), (5, 13), (12, 25)])
def test_softargmin_backward_edge_shapes(D, h, w):
    """train2d_ops.SoftArgmin at hw = 63, 65, 300 and small / odd D against float64 autograd, at test_softargmin_backward's tolerance
    (tests/test_train2d_gpu.py: depth 1e-5, gradient 5e-4 of the largest reference magnitude)."""
    from cds_mvsnet_amd import train2d_ops as t2
    torch.manual_seed(D * 1000 + h * w)
    pre = torch.randn(2, D, h, w, dtype=torch.float64) * 3
    hyp = torch.rand(2, D, h, w, dtype=torch.float64) * 100 + 400
    pre, hyp = pre.float().double(), hyp.float().double()          # the fp32 numbers the kernel sees
    pr = pre.clone().requires_grad_(True)
    dr = (F.softmax(pr, dim=1) * hyp).sum(dim=1)
    g = torch.randn_like(dr)
    dr.backward(g)
    pg = pre.float().to(DEV).requires_grad_(True)
    d = t2.SoftArgmin.apply(pg, hyp.float().to(DEV))
    d.backward(g.float().to(DEV))
    _close(d, dr, "depth", rel=1e-5)
    _close(pg.grad, pr.grad, "dpre", rel=5e-4)


# ------------------------------------------------------------------------------------------------
# K6
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.K6_CASES, ids=lambda c: "D%d-%dx%d-s%d-p%d" % c)
def test_k6_hypotheses_vs_float64(case, ops):
    D, H, W, scale, div = case
    dmin, dmax = R.K6_RANGE
    worst = (0.0, 0.0)
    for interval in R.K6_INTERVALS:
        for variant in R.K6_VARIANTS:
            prev = R.k6_prev(variant, D, H, W, div, interval)
            ref = R.hypotheses64(prev, D, interval, dmin, dmax, H, W, scale)
            bar, e32 = R.fp32_bar(ref, R.hypotheses(prev, D, interval, dmin, dmax, H, W, scale, torch.float32), scale=dmax)
            prev_d = prev.to(DEV).contiguous()
            out_d = ops.depth_hypotheses(prev_d, D, H, W, scale, interval, dmin, dmax)
            block = torch.tensor([interval, dmin, dmax], dtype=torch.float32).to(DEV)        # the device geometry form
            out_g = ops.depth_hypotheses(prev_d, D, H, W, scale, block[:1], block[1:])
            tag = (interval, variant)
            assert out_d.shape == (D, H // scale, W // scale), tag
            assert torch.equal(out_d, out_g), tag
            assert torch.equal(out_d, ops.depth_hypotheses(prev_d, D, H, W, scale, interval, dmin, dmax)), tag
            out = out_d.cpu()
            err = float((out.double() - ref).abs().max())
            worst = (max(worst[0], err / bar), max(worst[1], _ratio(err, e32)))
            print(f"K6 {case} interval={interval} {variant}: {err:.2e} (torch {e32:.2e}, bar {bar:.2e})")
            assert err <= bar, (tag, err, bar)
            lo, hi = R.hypotheses_clamped64(prev, D, interval, dmin, dmax, H, W, scale, dmax * 2.0 ** -22)
            assert bool((out[lo] == dmin).all()) and bool((out[hi] == dmax).all()), tag
            assert float(out.min()) >= dmin and float(out.max()) <= dmax, tag
    print("RATIO K6 %s hyp=%.3f/%.3f" % (case, worst[0], worst[1]))


@pytest.mark.parametrize("D", [2, 3, 48, 192])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 13)])
def test_k6_depth_planes_bit_equal(D, h, w, ops):
    for lo, hi in ((425.0, 902.5), (170.3, 361.9)):
        want = R.planes(lo, hi, D, h, w, torch.float32)
        got = ops.depth_planes(D, h, w, lo, hi, DEV)
        rng = torch.tensor([lo, hi], dtype=torch.float32).to(DEV)
        assert torch.equal(got.cpu(), want), (lo, hi)
        assert torch.equal(got, ops.depth_planes(D, h, w, rng, None, DEV)), (lo, hi)
        assert bool((got[0].cpu() == torch.tensor(lo, dtype=torch.float32)).all())
        assert float((got.cpu().double() - R.planes64(float(torch.tensor(lo)), float(torch.tensor(hi)), D, h, w)).abs().max()) \
            <= (D + 2) * 2.0 ** -15                                # the forward bound of test_regress_ref_cpu.py


# ------------------------------------------------------------------------------------------------
# volume_normalize_: the scalar tail of the planar kernel (hw % 4 != 0) and the channels-last form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True])
def test_volume_normalize_hw63(channels_last, ops):
    """volume / (vis_sum + 1e-6) (model.py:74) at hw = 63 against float64, within 1 ulp (2^-23 relative): one rounding of the sum, one
    of the quotient, half an ulp each; where no view sees the pixel the sum is exact and the divisor is the fp32 number nearest 1e-6
    (2.5e-9 away, relatively)."""
    g = torch.Generator().manual_seed(63)
    C, D, h, w = (8, 3, 7, 9) if channels_last else (3, 5, 7, 9)
    vol = torch.randn(C, D, h, w, generator=g)
    vs = 0.25 + 3.0 * torch.rand(h, w, generator=g)
    vs[0, 0] = 0.0                                                   # a pixel no view sees: the 1e-6 is all that divides
    ref = vol.double() / (vs.double() + 1e-6)
    if channels_last:
        got = ops.volume_normalize_(vol.permute(1, 2, 3, 0).contiguous().to(DEV), vs.to(DEV), channels_last=True).permute(3, 0, 1, 2)
    else:
        got = ops.volume_normalize_(vol.clone().to(DEV), vs.to(DEV))
    rel = float(((got.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-300)).max())
    print(f"RATIO VN cl={int(channels_last)} rel={rel / R.U23:.3f}")
    assert rel <= R.U23
