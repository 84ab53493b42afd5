"""The z-marching form of the deep stride-1 CostRegNet layers in split-f16 arithmetic (csrc/conv3d_zmg.hip: conv4 32 -> 32 with the
K dimension split over four waves, conv6 64 -> 64 with two 8-channel rounds per wave and the cout blocks split over gridDim.y),
forced with CDS_ZMG_DEEP=2 whatever the volume's size.  The bar is that of test_conv3d_split_f16_is_fp32_class: against a float64
convolution evaluated by PyTorch on the CPU no worse than 1.5x a plain fp32 evaluation + one ulp of the result scale."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# shapes that cut the 16 x 4 / 16 x 2 columns in x, y and z; the M1 deep volumes themselves (level 2 / level 3 of 192 x 512 x 640)
SHAPES = {32: [(5, 9, 20), (9, 13, 70), (6, 11, 37), (48, 128, 160)],
          64: [(5, 9, 20), (9, 13, 70), (6, 11, 37), (24, 64, 80)]}
CASES = [(c, s, None) for c in (32, 64) for s in SHAPES[c]] + [(32, (21, 13, 40), 4), (64, (21, 13, 40), 4), (64, (9, 13, 70), 3)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cds_mvsnet_amd import ops as o
    assert o.version() >= 100
    return o


@pytest.mark.parametrize("loose", [1.0, 6.5])
@pytest.mark.parametrize("c,shape,nseg", CASES)
def test_deep_zmarch_split_f16_is_fp32_class(c, shape, nseg, loose, ops, monkeypatch):
    """conv4 / conv6 on the z-march: error against float64 <= 1.5x the fp32 error + 1 ulp (with and without ReLU, with a loose input
    bound), out_bound == the exact maximum magnitude stored, two runs bit-equal (the partial sums of the K split are added in a fixed
    order).  nseg: that many z segments per column (CDS_ZMG_NSEG).  Printed, not asserted: the distance to the tiled kernel."""
    if not ops.USE_SPLIT_F16:
        pytest.skip("CDS_SPLIT_F16=0: the split-f16 convolution entry is switched off")
    D, H, W = shape
    assert ops.conv3d_sf16_supported(c, c, 1)
    g = torch.Generator().manual_seed(c * 100 + c + D)
    x = torch.randn(c, D, H, W, generator=g) * torch.exp(torch.randn(c, 1, 1, 1, generator=g))     # uneven channel scales
    w = torch.randn(c, c, 3, 3, 3, generator=g) / (27 * c) ** 0.5
    b = torch.randn(c, generator=g)
    want64 = F.conv3d(x.double().unsqueeze(0), w.double(), b.double(), padding=1)[0]
    want32 = F.conv3d(x.unsqueeze(0), w, b, padding=1)[0]
    wh, w_inv = ops.split_pack_conv3d(w.to(DEV), f16=True)
    x_cl = x.permute(1, 2, 3, 0).contiguous().to(DEV)
    in_bound = (x_cl.abs().amax() * loose).reshape(1)
    wpk = w.permute(1, 2, 3, 4, 0).reshape(c, 27, c).contiguous().to(DEV)
    chain32 = ops.conv3d_k3(x.to(DEV), wpk, b.to(DEV), stride=1, relu=False).cpu()
    err_f32 = max((want32.double() - want64).abs().max().item(), (chain32.double() - want64).abs().max().item())
    ulp = want64.abs().max().item() * 2.0 ** -23

    def run(deep, relu, ob=None):
        monkeypatch.setenv("CDS_ZMG_DEEP", str(deep))
        if nseg and deep:
            monkeypatch.setenv("CDS_ZMG_NSEG", str(nseg))
        else:
            monkeypatch.delenv("CDS_ZMG_NSEG", raising=False)
        return ops.conv3d_sbf(x_cl, wh, b.to(DEV), c, stride=1, relu=relu, in_bound=in_bound, w_inv_scale=w_inv, out_bound=ob)

    for relu in (False, True):
        out_bound = torch.zeros(1, device=DEV)
        got = run(2, relu, out_bound)
        again = run(2, relu)
        tiled = run(0, relu)
        torch.cuda.synchronize()
        assert float(out_bound) == float(got.abs().max()), (relu, float(out_bound), float(got.abs().max()))
        assert torch.equal(got, again), "two runs of the z-march differ"
        ref64 = want64.clamp_min(0) if relu else want64
        err = (got.cpu().permute(3, 0, 1, 2).double() - ref64).abs().max().item()
        err_t = (tiled.cpu().permute(3, 0, 1, 2).double() - ref64).abs().max().item()
        print(f"conv3d {c}->{c} {D}x{H}x{W} nseg {nseg} bound x{loose} relu {int(relu)}: max err vs float64: z-march {err:.2e}, tiled {err_t:.2e}, "
              f"fp32 {err_f32:.2e}; max |z-march - tiled| {(got - tiled).abs().max().item():.2e}")
        assert err <= 1.5 * err_f32 + ulp, (relu, err, err_f32)


def test_deep_zmarch_auto_keeps_small_volumes_tiled(ops, monkeypatch):
    """CDS_ZMG_DEEP=1 (the default) sends a volume of a handful of columns to the tiled kernel: bit-equal to CDS_ZMG_DEEP=0."""
    if not ops.USE_SPLIT_F16:
        pytest.skip("CDS_SPLIT_F16=0: the split-f16 convolution entry is switched off")
    g = torch.Generator().manual_seed(5)
    x_cl = torch.randn(8, 16, 32, 32, generator=g).to(DEV)
    w = torch.randn(32, 32, 3, 3, 3, generator=g) / (27 * 32) ** 0.5
    wh, w_inv = ops.split_pack_conv3d(w.to(DEV), f16=True)
    in_bound = x_cl.abs().amax().reshape(1)
    outs = []
    for deep in ("0", "1"):
        monkeypatch.setenv("CDS_ZMG_DEEP", deep)
        outs.append(ops.conv3d_sbf(x_cl, wh, None, 32, stride=1, relu=True, in_bound=in_bound, w_inv_scale=w_inv))
    assert torch.equal(outs[0], outs[1])
