"""Split-f16 inference layers (csrc/sbf_common.hpp: one power-of-two scale per tensor, from a bound on max |x|) where that scale is
set by a few values far above the bulk, and with the loose bounds the model really passes.

Outliers: for each inference entry point one representative shape per kernel family, inputs with 0.1 % of the entries at 10^3 x the
bulk or a single 10^4 x spike, the bound = the true maximum.  The error is measured on the outputs whose receptive field holds no
outlier, against float64: <= 1.5 x the fp32 error on the same outputs + one ulp of THEIR scale (test_train_sf16_gpu._check with a mask;
the whole tensor's scale would make the ulp term swamp the bulk).  The 2D layers see their input after the pending affine: the affine
here is the identity (slope 1); the DynamicConv blend is made uniform (second attention layer 0) so that the output is the mean of
the branches.
Full resolution: the FeatureNet of the model at 1184x1600 with the x_bound it passes (sqrt(H W) of an InstanceNorm-ed map, ~2^8
above the true maximum), conv01 and downsample1 checked on six 64x64 output windows against float64 on input crops with the halo."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
KINDS = ["sparse_1e3", "spike_1e4"]


def _check(name, got, r64, r32, mask=None, f32=None):
    """err(got) <= 1.5 x the fp32 error + one ulp of the (masked) reference scale; the fp32 error: PyTorch's and, when given, the
    library's exact-fp32 kernel's, the larger.  Non-finite values fail before any error is computed."""
    assert torch.isfinite(got).all(), (name, "non-finite output")
    if mask is not None:
        assert mask.shape == got.shape and mask.float().mean() > 0.05, (name, "no bulk left to measure")
        got, r64, r32 = got[mask], r64[mask], r32[mask]
        f32 = f32[mask] if f32 is not None else None
    err = (got.double() - r64).abs().max().item()
    err32 = (r32.double() - r64).abs().max().item()
    if f32 is not None:
        err32 = max(err32, (f32.double() - r64).abs().max().item())
    ulp = r64.abs().max().item() * 2.0 ** -23
    print(f"{name}: split-f16 {err:.3e}, fp32 {err32:.3e}, ulp {ulp:.1e}, ratio {err / err32 if err32 else float('inf'):.2f}")
    assert np.isfinite(err) and err <= 1.5 * err32 + ulp, (name, err, err32)
    return err, err32


def _outliers(shape, kind, seed):
    """randn bulk with outliers -> (x, mask of the outlier entries)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if kind == "sparse_1e3":
        spikes = torch.rand(shape, generator=g) < 1e-3
        x[spikes] *= 1e3
    else:
        spikes = torch.zeros(shape, dtype=torch.bool)
        spikes.view(-1)[x.numel() // 3] = True
        x[spikes] = 1e4
    return x, spikes


# ------------------------------------------------------------------------------------------------------------------------------------
# CostRegNet: conv3d_sbf (pair conv0, stride-2 conv1, tiled conv6), deconv3d_sbf (conv7), deconv3d_zm (conv9), deconv_prob_zm (conv11)
# ------------------------------------------------------------------------------------------------------------------------------------
CONV3D = [("conv0", 8, 8, 101, (50, 9, 70)), ("conv1", 8, 16, 2, (21, 37, 131)), ("conv6", 64, 64, 1, (6, 11, 37))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layer,cin,cout,code,vol", CONV3D)
def test_conv3d_outliers_keep_the_bulk_fp32_class(layer, cin, cout, code, vol, kind):
    from cds_mvsnet_amd import ops
    assert ops.conv3d_sf16_supported(cin, cout, code)
    x, spikes = _outliers((cin,) + vol, kind, seed=cin * 7 + cout)
    g = torch.Generator().manual_seed(3)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    b = torch.randn(cout, generator=g)
    stride = 1 if code == ops.SBF_PAIR else code
    r64 = F.conv3d(x.double()[None], w.double(), b.double(), stride=stride, padding=1)[0].clamp_min(0)
    r32 = F.conv3d(x[None], w, b, stride=stride, padding=1)[0].clamp_min(0)
    wpk = w.permute(1, 2, 3, 4, 0).reshape(cin, 27, cout).contiguous().to(DEV)
    f32 = ops.conv3d_k3(x.to(DEV), wpk, b.to(DEV), stride=stride, relu=True).cpu()
    wh, winv = (ops.split_pack_conv3d_pair if code == ops.SBF_PAIR else ops.split_pack_conv3d)(w.to(DEV), f16=True)
    x_cl = x.permute(1, 2, 3, 0).contiguous().to(DEV)
    ob = torch.zeros(1, device=DEV)
    got = ops.conv3d_sbf(x_cl, wh, b.to(DEV), cout, stride=code, relu=True, in_bound=x_cl.abs().amax().reshape(1), w_inv_scale=winv,
                         out_bound=ob)
    torch.cuda.synchronize()
    got = got.cpu().permute(3, 0, 1, 2)
    reach = F.max_pool3d(spikes.any(0, keepdim=True)[None].float(), 3, stride, 1)[0].bool().expand_as(r64)
    _check(f"{layer} {cin}->{cout} {kind} bulk", got, r64, r32, mask=~reach, f32=f32)
    assert float(ob) == got.abs().max().item()


def _reach_transposed(spikes_any, out_shape):
    """Outputs of a ConvTranspose3d k3 s2 p1 op1 that an input voxel marked in spikes_any [D,H,W] contributes to."""
    r = F.conv_transpose3d(spikes_any[None, None].float(), torch.ones(1, 1, 3, 3, 3), stride=2, padding=1, output_padding=1)[0, 0] > 0
    assert r.shape == out_shape
    return r


DECONV = [("conv7", 64, 32, (5, 9, 37)), ("conv9", 32, 16, (7, 13, 37)), ("conv11", 16, 8, (6, 20, 33))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layer,cin,cout,vol", DECONV)
def test_deconv3d_outliers_keep_the_bulk_fp32_class(layer, cin, cout, vol, kind):
    """conv7 (tiled transposed kernel), conv9 (z-marching class-per-wave kernel), conv11 + residual + prob (fused): ReLU and the
    residual as the network runs them."""
    from cds_mvsnet_amd import ops
    x, spikes = _outliers((cin,) + vol, kind, seed=cin * 5 + cout)
    g = torch.Generator().manual_seed(4)
    w = torch.randn(cin, cout, 3, 3, 3, generator=g) / (27 * cin / 8) ** 0.5
    b = torch.randn(cout, generator=g)
    D, H, W = vol
    skip = torch.randn(cout, 2 * D, 2 * H, 2 * W, generator=g)
    wp = torch.randn(1, cout, 3, 3, 3, generator=g) / 27 ** 0.5

    def ref(dtype):
        y = F.conv_transpose3d(x.to(dtype)[None], w.to(dtype), b.to(dtype), stride=2, padding=1, output_padding=1).clamp_min(0)
        y = y + skip.to(dtype)[None]
        return F.conv3d(y, wp.to(dtype), padding=1)[0] if layer == "conv11" else y[0]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    x_cl = x.permute(1, 2, 3, 0).contiguous().to(DEV)
    skip_cl = skip.permute(1, 2, 3, 0).contiguous().to(DEV)
    bound = x_cl.abs().amax().reshape(1)
    wpk = w.permute(0, 2, 3, 4, 1).reshape(cin, 27, cout).contiguous().to(DEV)
    f32 = ops.deconv3d_k3s2(x.to(DEV), wpk, b.to(DEV), relu=True, skip=skip.to(DEV))
    ob = torch.zeros(1, device=DEV)
    if layer == "conv7":
        wh, winv = ops.split_pack_deconv3d(w.to(DEV), f16=True)
        got = ops.deconv3d_sbf(x_cl, wh, b.to(DEV), cout, skip=skip_cl, in_bound=bound, w_inv_scale=winv, out_bound=ob)
    elif layer == "conv9":
        wh, winv = ops.split_pack_deconv_cls(w.to(DEV), f16=True)
        got = ops.deconv3d_zm(x_cl, wh, b.to(DEV), skip=skip_cl, in_bound=bound, w_inv_scale=winv, out_bound=ob)
    else:
        wh, winv = ops.split_pack_deconv_prob(w.to(DEV), f16=True)
        got = ops.deconv_prob_zm(x_cl, wh, b.to(DEV), skip_cl, ops.pack_prob_table(wp.to(DEV)), in_bound=bound, w_inv_scale=winv)
        f32 = ops.conv3d_k3(f32, wp.permute(1, 2, 3, 4, 0).reshape(cout, 27, 1).contiguous().to(DEV), None, relu=False)
    torch.cuda.synchronize()
    got = got.cpu()
    got = got[None] if layer == "conv11" else got.permute(3, 0, 1, 2)
    reach = _reach_transposed(spikes.any(0), tuple(r64.shape[1:]))
    if layer == "conv11":                        # prob: 3 x 3 x 3 more
        reach = F.max_pool3d(reach[None, None].float(), 3, 1, 1)[0, 0].bool()
    _check(f"{layer} {cin}->{cout} {kind} bulk", got, r64, r32, mask=~reach.expand_as(r64), f32=f32.cpu())
    if layer != "conv11":
        assert float(ob) == got.abs().max().item()


# ------------------------------------------------------------------------------------------------------------------------------------
# FeatureNet: dynconv_cl, conv2d_k3s2_cl (x_bound), conv00_cl (in_bound)
# ------------------------------------------------------------------------------------------------------------------------------------
THIRD = float(torch.tensor(1.0 / 3.0, dtype=torch.float32))     # the blend weight of three branches with equal logits


def _identity_affine(N, C):
    return torch.tensor([1.0, 0.0, 1.0]).repeat(N, C, 1).contiguous()


def _dyn_weights(c, ks, g):
    """Branch weights [C + 3, C, k, k] (att channels included) and a blend MLP whose second layer is 0: equal logits, weights 1/3."""
    K = len(ks)
    ws = [torch.randn(c + 3, c, k, k, generator=g) / (c * k * k) ** 0.5 for k in ks]
    w1, b1, w2 = torch.randn(4, K, generator=g), torch.randn(4, generator=g), torch.zeros(K, 4)
    return ws, w1, b1, w2


@pytest.mark.parametrize("kind", KINDS)
def test_dynconv_cl_outliers_keep_the_bulk_fp32_class(kind):
    from cds_mvsnet_amd import ops
    c, ks, N, H, W = 8, (3, 5, 7), 2, 21, 44
    x, spikes = _outliers((N, c, H, W), kind, seed=81)
    g = torch.Generator().manual_seed(82)
    ws, w1, b1, w2 = _dyn_weights(c, ks, g)
    epi = torch.tensor([[W * 0.3 + 5.0 * n, -H * 1.7 - n] for n in range(N)], dtype=torch.float32)
    wh, winv = ops.split_pack_dynconv([w.to(DEV) for w in ws], f16=True)
    x_cl = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    got = ops.dynconv_cl(x_cl, wh, None, ks, w1.to(DEV), b1.to(DEV), w2.to(DEV), epi, 1.0, 0.1, in_affine=_identity_affine(N, c).to(DEV),
                         x_bound=float(x.abs().max()), w_inv_scale=winv)[0]
    torch.cuda.synchronize()
    got = got.cpu().permute(0, 3, 1, 2)
    r64 = sum(THIRD * F.conv2d(x.double(), w[:c].double(), padding=(k - 1) // 2) for w, k in zip(ws, ks))
    r32 = sum(THIRD * F.conv2d(x, w[:c], padding=(k - 1) // 2) for w, k in zip(ws, ks))
    reach = F.max_pool2d(spikes.any(1, keepdim=True).float(), max(ks), 1, max(ks) // 2).bool().expand_as(r64)
    _check(f"dynconv_cl {c} {ks} {kind} bulk", got, r64, r32, mask=~reach)


@pytest.mark.parametrize("kind", KINDS)
def test_downsample_cl_outliers_keep_the_bulk_fp32_class(kind):
    from cds_mvsnet_amd import ops
    cin, cout, N, H, W = 8, 16, 2, 70, 133
    x, spikes = _outliers((N, cin, H, W), kind, seed=91)
    w = torch.randn(cout, cin, 3, 3, generator=torch.Generator().manual_seed(92)) / (cin * 9) ** 0.5
    wh, winv = ops.split_pack_dynconv([w.to(DEV)], f16=True)
    x_cl = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    got = ops.conv2d_k3s2_cl(x_cl, None, cout, _identity_affine(N, cin).to(DEV), wsplit=wh, w_inv_scale=winv, x_bound=float(x.abs().max()))
    torch.cuda.synchronize()
    got = got.cpu().permute(0, 3, 1, 2)
    r64 = F.conv2d(x.double(), w.double(), stride=2, padding=1)
    r32 = F.conv2d(x, w, stride=2, padding=1)
    reach = F.max_pool2d(spikes.any(1, keepdim=True).float(), 3, 2, 1).bool().expand_as(r64)
    _check(f"conv2d_k3s2_cl {cin}->{cout} {kind} bulk", got, r64, r32, mask=~reach)


@pytest.mark.parametrize("kind", KINDS)
def test_conv00_outliers_keep_the_bulk_fp32_class(kind):
    from cds_mvsnet_amd import ops
    N, n_shared, H, W = 3, 1, 40, 70
    x, spikes = _outliers((N, 3, H, W), kind, seed=71)
    x = x.abs()                                          # images: non-negative
    ks = (3, 7, 11)
    g = torch.Generator().manual_seed(72)
    ws = [torch.cat((torch.randn(8, 3, k, k, generator=g) / (3 * k * k) ** 0.5, torch.randn(3, 3, k, k, generator=g) * 0.1)) for k in ks]
    w1, b1, w2 = torch.randn(4, 3, generator=g), torch.randn(4, generator=g), torch.zeros(3, 4)    # equal logits: weights 1/3
    epi = torch.tensor([[W * 0.4 + 3.0 * n, H * 2.1 + n] for n in range(N)], dtype=torch.float32)
    wh, winv = ops.split_pack_conv00([w.to(DEV) for w in ws], f16=True)
    got = ops.conv00_cl(x.to(DEV), wh, None, w1.to(DEV), b1.to(DEV), w2.to(DEV), epi, 1.0, n_shared, 0.1,
                        in_bound=x.abs().amax().reshape(1).to(DEV), w_inv_scale=winv)[0]
    torch.cuda.synchronize()
    got = got.cpu().permute(0, 3, 1, 2)
    r64 = sum(THIRD * F.conv2d(x.double(), w[:8].double(), padding=(k - 1) // 2) for w, k in zip(ws, ks))
    r32 = sum(THIRD * F.conv2d(x, w[:8], padding=(k - 1) // 2) for w, k in zip(ws, ks))
    reach = F.max_pool2d(spikes.any(1, keepdim=True).float(), 11, 1, 5).bool().expand_as(r64)
    _check(f"conv00_cl {kind} bulk", got, r64, r32, mask=~reach)


# ------------------------------------------------------------------------------------------------------------------------------------
# the bounds model.py passes, at full resolution
# ------------------------------------------------------------------------------------------------------------------------------------
def _windows(H, W, s=64):
    """Six s x s output windows: the four corners, the middle of the top edge, the centre."""
    return [(0, 0), (0, W - s), (H - s, 0), (H - s, W - s), (0, (W - s) // 2), ((H - s) // 2, (W - s) // 2)]


def _post_affine(x, aff, dtype):
    """x [N,C,h,w] after its pending affine (scale, shift, LeakyReLU slope) in ``dtype``."""
    a = aff.to(dtype)
    y = x.to(dtype) * a[:, :, 0, None, None] + a[:, :, 1, None, None]
    return torch.where(y > 0, y, y * a[:, :, 2, None, None])


def test_full_resolution_feature_layers_with_the_model_bounds():
    """FeatureNet at N = 1, 1184x1600 through the model's own runner: conv01 (DynamicConv 8, kernel sizes 3 / 5 / 7) and downsample1
    (8 -> 16, stride 2) receive x_bound = sqrt(H W) ~ 1376 from model.py for an InstanceNorm-ed input whose real maximum is O(5).  On six
    64x64 output windows against float64 (input crops with the kernel's halo): <= 1.5 x PyTorch fp32's error + one ulp."""
    import cds_mvsnet_amd.model as cm
    from cds_mvsnet_amd import FeatureNet, ops, seeded_init_, synth
    assert ops.USE_SPLIT_F16
    H, W = 1184, 1600
    net = seeded_init_(FeatureNet(8), 5)
    with torch.no_grad():
        net.conv01.conv.att_weights[3].weight.zero_()       # equal logits: conv01's blend is the mean of its three branches
    net = net.to(DEV).eval()
    imgs = synth.make_images(1, H, W, seed=6)[0].to(DEV)
    epi = torch.tensor([[W * 0.4, -H * 1.3]], dtype=torch.float32)
    seen = {}

    def spy(name):
        orig = getattr(ops, name)

        def f(x, *args, **kw):
            out = orig(x, *args, **kw)
            if x.shape[1:3] == (H, W) and name not in seen:
                torch.cuda.synchronize()
                seen[name] = (x, args, kw, out[0] if isinstance(out, tuple) else out)
            return out
        return orig, f

    saved = {}
    for name in ("dynconv_cl", "conv2d_k3s2_cl"):
        saved[name], f = spy(name)
        setattr(ops, name, f)
    try:
        with torch.no_grad():
            cm._FeatureRunner(net)(imgs, epi, 0.01, n_chw=1, n_shared=1)
        torch.cuda.synchronize()
    finally:
        for name, orig in saved.items():
            setattr(ops, name, orig)
    assert set(seen) == {"dynconv_cl", "conv2d_k3s2_cl"}, set(seen)

    # conv01
    x, args, kw, out = seen["dynconv_cl"]
    assert kw.get("x_bound") is not None and tuple(args[2]) == (3, 5, 7), "conv01 did not run in split-f16"
    dc = net.conv01.conv
    aff = kw["in_affine"].cpu()
    xin = x.permute(0, 3, 1, 2).cpu()
    true_max = _post_affine(xin, aff, torch.float64).abs().max().item()
    assert kw["x_bound"] >= true_max
    print(f"conv01: x_bound {kw['x_bound']:.1f}, max |input after affine| {true_max:.3f}")
    got = out.permute(0, 3, 1, 2).cpu()
    assert torch.isfinite(got).all(), "conv01: non-finite output"
    ws = [dc.convs[i].weight.detach().cpu() for i in range(3)]
    for y0, x0 in _windows(H, W):
        crop = {}
        for dtype in (torch.float64, torch.float32):
            xp = F.pad(_post_affine(xin, aff, dtype), (3, 3, 3, 3))[:, :, y0:y0 + 70, x0:x0 + 70]
            # the crop starts 3 rows / columns before the window: kernel k (half width r) reads crop rows 3 - r .. 66 + r
            crop[dtype] = sum(THIRD * F.conv2d(xp[:, :, 3 - r:67 + r, 3 - r:67 + r], w.to(dtype)) for w, r in zip(ws, (1, 2, 3)))
        _check(f"conv01 full-res window ({y0},{x0})", got[:, :, y0:y0 + 64, x0:x0 + 64], crop[torch.float64], crop[torch.float32])

    # downsample1
    x, args, kw, out = seen["conv2d_k3s2_cl"]
    assert kw.get("x_bound") is not None and kw.get("wsplit") is not None, "downsample1 did not run in split-f16"
    aff = args[2].cpu() if len(args) > 2 else kw["in_affine"].cpu()
    xin = x.permute(0, 3, 1, 2).cpu()
    true_max = _post_affine(xin, aff, torch.float64).abs().max().item()
    assert kw["x_bound"] >= true_max
    print(f"downsample1: x_bound {kw['x_bound']:.1f}, max |input after affine| {true_max:.3f}")
    got = out.permute(0, 3, 1, 2).cpu()
    assert torch.isfinite(got).all(), "downsample1: non-finite output"
    w = net.downsample1.conv.weight.detach().cpu()
    Ho, Wo = got.shape[2:]
    for y0, x0 in _windows(Ho, Wo):
        crop = {}
        for dtype in (torch.float64, torch.float32):
            xp = F.pad(_post_affine(xin, aff, dtype), (1, 1, 1, 1))[:, :, 2 * y0:2 * y0 + 129, 2 * x0:2 * x0 + 129]
            crop[dtype] = F.conv2d(xp, w.to(dtype), stride=2)
        _check(f"downsample1 full-res window ({y0},{x0})", got[:, :, y0:y0 + 64, x0:x0 + 64], crop[torch.float64], crop[torch.float32])
