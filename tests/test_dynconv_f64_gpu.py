"""The inference DynamicConv kernels against float64 (tests/dynconv_ref.py), per kernel, at edge shapes.

Every kernel that applies the blend epilogue of csrc/feat_common.hpp (blend_from_att) - the planar blend kernels, the channels-last blend,
the planar fused matrix-core kernel, the channels-last DynamicConv in split-bf16 and split-f16 and conv00 in both - is held to
|kernel - float64| <= bound at EVERY pixel of out and norm_curv, the bound being the a-priori one of dynconv_ref.bound() (PyTorch's own
fp32 evaluation needs half of it: tests/test_dynconv_ref_cpu.py).  The older tests compare these kernels with one another, and all of them
include the same header: an error in the shared epilogue passes those bit for bit.

Cases (dynconv_ref.*_CASES): K = 2 and K = 3, C = 8 / 11 / 16 / 32, a non-zero second attention layer, bias on the response channels,
in_affine with negative scales, shared slots n_shared in {1, 2, N}, epipoles outside / on a pixel centre / sub-pixel inside / on the
half-pixel border / 3e7 pixels away, T = 1, 0.01, 0.001; sizes either side of the blend kernels' 1024-pixel block and around the 32 x 8
tile of the matrix-core kernels (1 x 1 and 3 x 2 included).  Every (stats, affine) a call returns is checked against the float64 sums of
the kernel's own output.  cds_dynconv_blend_f32 has no wrapper in ops.py and is not covered (it forwards to the shared-slot kernel)."""
import pytest
import torch

import dynconv_ref as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from cds_mvsnet_amd import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    for name in sorted(D.RATIOS):
        print(f"worst |kernel - float64| / bound, {name}: {D.RATIOS[name]:.3f}")


def _mlp(case, dev):
    return case["w1"].to(dev), case["b1"].to(dev), case["w2"].to(dev)


def _opt(t, dev):
    return None if t is None else t.to(dev)


def _chw(x_cl):
    return x_cl.permute(0, 3, 1, 2).cpu()


def _refs(case):
    return {T: D.ref_and_bound(case, T) for T in D.TEMPS}


@pytest.mark.parametrize("K,c,H,W,N,n_shared", D.BLEND_CASES)
def test_blend_kernels_from_exact_branches(K, c, H, W, N, n_shared, dev, ops):
    """cds_dynconv_blend_shared_f32, cds_dynconv_blend_stats_f32 and (K = 3, 8 channels: the shape it is built for)
    cds_dynconv_blend_cl_f32 on an exact branch tensor: the epilogue alone, e_br = 0."""
    case = D.blend_case(K, c, H, W, N, n_shared)
    br = case["branches"].to(dev)
    w1, b1, w2 = _mlp(case, dev)
    for T, (r64, b) in _refs(case).items():
        o, n = ops.dynconv_blend(br, w1, b1, w2, case["epi"], T, n_shared)
        D.check(o.cpu(), n.cpu(), r64, b, "dynconv_blend (shared)")
        o, n, st, af = ops.dynconv_blend(br, w1, b1, w2, case["epi"], T, n_shared, stats_slope=0.1)
        D.check(o.cpu(), n.cpu(), r64, b, "dynconv_blend (stats)")
        D.check_stats(o.cpu(), st.cpu(), af.cpu(), 0.1, ("dynconv_blend (stats)", T))
        if (K, c) == (3, 8):
            o, n, st, af = ops.dynconv_blend_cl(br, w1, b1, w2, case["epi"], T, n_shared, 0.1)
            assert tuple(o.shape) == (N, H, W, c)
            D.check(_chw(o), n.cpu(), r64, b, "dynconv_blend_cl")
            D.check_stats(_chw(o), st.cpu(), af.cpu(), 0.1, ("dynconv_blend_cl", T))
    if (K, c) != (3, 8):
        with pytest.raises(ValueError):
            ops.dynconv_blend_cl(br, w1, b1, w2, case["epi"], 1.0, n_shared, 0.1)


def test_blend_rejects_what_it_has_no_kernel_for(dev, ops):
    case = D.make_blend_case(1, 4, 8, 2, 1, 3, 5)
    with pytest.raises(ValueError):
        ops.dynconv_blend(case["branches"].to(dev), torch.zeros(4, 4, device=dev), torch.zeros(4, device=dev), torch.zeros(4, 4, device=dev),
                          case["epi"], 1.0, 1)
    case = D.make_conv_case(2, 8, 8, (1, 3), 1, 1, 5, 6, False, False)
    ws = ops.split_pack_dynconv([w.to(dev) for w in case["ws"]])
    with pytest.raises(ValueError):                  # the planar matrix-core kernel needs whole 16-byte row groups: W % 4 == 0
        ops.dynconv_fused_sbf(case["x"].to(dev), ws, None, 8, (1, 3), *_mlp(case, dev), case["epi"], 1.0, 0.1)


@pytest.mark.parametrize("c,ks,H,W,aff", D.FUSED_CASES)
def test_fused_sbf_kernel(c, ks, H, W, aff, dev, ops):
    """cds_dynconv_fused_sbf_f32: every instantiation (branches x 16-column blocks), with and without the pending affine."""
    case = D.fused_case(c, ks, H, W, aff)
    ws = ops.split_pack_dynconv([w.to(dev) for w in case["ws"]])
    x, a, bs = case["x"].to(dev), _opt(case["in_affine"], dev), case["bias"].to(dev)
    w1, b1, w2 = _mlp(case, dev)
    for T, (r64, b) in _refs(case).items():
        o, n, st, af = ops.dynconv_fused_sbf(x, ws, bs, c, ks, w1, b1, w2, case["epi"], T, 0.1, in_affine=a)
        D.check(o.cpu(), n.cpu(), r64, b, "dynconv_fused_sbf")
        D.check_stats(o.cpu(), st.cpu(), af.cpu(), 0.1, ("dynconv_fused_sbf", T))


@pytest.mark.parametrize("c,ks,H,W,N", D.CL_CASES)
def test_dynconv_cl_kernels(c, ks, H, W, N, dev, ops):
    """cds_dynconv_cl_f32 (split-bf16) and cds_dynconv_cl_sf16_f32 with x_bound = max |x after its affine| and 8 x that (the model passes
    a loose bound), a non-trivial blend, the pending affine with negative scales."""
    assert D.CL_SHAPES == ops.DYNCONV_CL_SHAPES
    case = D.cl_case(c, ks, H, W, N)
    wdev = [w.to(dev) for w in case["ws"]]
    ws = ops.split_pack_dynconv(wdev)
    wh, winv = ops.split_pack_dynconv(wdev, f16=True)
    x_cl = case["x"].permute(0, 2, 3, 1).contiguous().to(dev)
    a, bs = case["in_affine"].to(dev), _opt(case["bias"], dev)
    w1, b1, w2 = _mlp(case, dev)
    xmax = D.post_affine(case["x"], case["in_affine"], torch.float64).abs().max().item()
    for T, (r64, b) in _refs(case).items():
        for name, kw in (("dynconv_cl split-bf16", {}), ("dynconv_cl split-f16", {"x_bound": xmax, "w_inv_scale": winv}),
                         ("dynconv_cl split-f16, 8 x bound", {"x_bound": 8.0 * xmax, "w_inv_scale": winv})):
            o, n, st, af = ops.dynconv_cl(x_cl, wh if kw else ws, bs, ks, w1, b1, w2, case["epi"], T, 0.1, in_affine=a, **kw)
            assert tuple(o.shape) == (N, H, W, c)
            D.check(_chw(o), n.cpu(), r64, b, name)
            D.check_stats(_chw(o), st.cpu(), af.cpu(), 0.1, (name, T))


@pytest.mark.parametrize("H,W,n_shared,bias", D.CONV00_CASES)
def test_conv00_cl_kernels(H, W, n_shared, bias, dev, ops):
    """cds_conv00_cl_f32 and cds_conv00_cl_sf16_f32 (in_bound = the images' maximum) on images in [0, 1], shared reference slots."""
    case = D.conv00_case(H, W, n_shared, bias)
    wdev = [w.to(dev) for w in case["ws"]]
    ws = ops.split_pack_conv00(wdev)
    wh, winv = ops.split_pack_conv00(wdev, f16=True)
    imgs, bs = case["x"].to(dev), _opt(case["bias"], dev)
    w1, b1, w2 = _mlp(case, dev)
    for T, (r64, b) in _refs(case).items():
        for name, kw in (("conv00_cl split-bf16", {}), ("conv00_cl split-f16", {"in_bound": imgs.abs().amax().reshape(1), "w_inv_scale": winv})):
            o, n, st, af = ops.conv00_cl(imgs, wh if kw else ws, bs, w1, b1, w2, case["epi"], T, n_shared, 0.1, **kw)
            assert tuple(o.shape) == (D.CONV00_N, H, W, 8)
            D.check(_chw(o), n.cpu(), r64, b, name)
            D.check_stats(_chw(o), st.cpu(), af.cpu(), 0.1, (name, T))
