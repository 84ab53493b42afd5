"""conv5 of CostRegNet (32 -> 64, stride 2) on the z-march in split-f16 arithmetic (csrc/conv3d_zmg.hip: 16 x 2 output columns on the
32-byte term-planar ring, K split in two with two 8-channel rounds per wave, four cout blocks), forced with CDS_ZMG_DEEP=2 whatever the
volume's size, and conv2 (16 -> 16) without its K split on the same ring layout.  The bar is that of tests/test_zmarch_deep_gpu.py:
against a float64 convolution evaluated by PyTorch on the CPU no worse than 1.5x a plain fp32 evaluation + one ulp of the result
scale."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CIN, COUT = 32, 64
LAYERS = {"conv5": (32, 64, 2), "conv2": (16, 16, 1)}       # cin, cout, stride

# input shapes that cut the 16 x 2 output columns and hit both stride parities in x, y and z; the last two with several z segments
CASES = [((5, 9, 20), None), ((6, 11, 37), None), ((9, 13, 70), None), ((8, 8, 32), None), ((7, 5, 33), None),
         ((21, 13, 40), 4), ((12, 20, 70), 3)]
# conv2: 32 x 8 columns cut in x, y and z, an odd and an even plane count, three z segments
CASES2 = [((3, 9, 20), None), ((5, 13, 70), None), ((4, 11, 37), None), ((9, 13, 40), 3)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cds_mvsnet_amd import ops as o
    assert o.version() >= 100
    return o


_REF = {}


def _case(layer, shape, ops):
    """Inputs, operands and the float64 / fp32 references of one shape: computed once, shared by the bound variants, never modified."""
    if (layer, shape) not in _REF:
        cin, cout, stride = LAYERS[layer]
        D, H, W = shape
        g = torch.Generator().manual_seed(5000 + 100 * D + H + W + cin)
        x = torch.randn(cin, D, H, W, generator=g) * torch.exp(torch.randn(cin, 1, 1, 1, generator=g))     # uneven channel scales
        w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
        b = torch.randn(cout, generator=g)
        want64 = F.conv3d(x.double().unsqueeze(0), w.double(), b.double(), stride=stride, padding=1)[0]
        want32 = F.conv3d(x.unsqueeze(0), w, b, stride=stride, padding=1)[0]
        wpk = w.permute(1, 2, 3, 4, 0).reshape(cin, 27, cout).contiguous().to(DEV)
        chain32 = ops.conv3d_k3(x.to(DEV), wpk, b.to(DEV), stride=stride, relu=False).cpu()
        err_f32 = max((want32.double() - want64).abs().max().item(), (chain32.double() - want64).abs().max().item())
        wh, w_inv = ops.split_pack_conv3d(w.to(DEV), f16=True)
        _REF[layer, shape] = dict(x_cl=x.permute(1, 2, 3, 0).contiguous().to(DEV), wh=wh, w_inv=w_inv, b=b.to(DEV), want64=want64,
                                  err_f32=err_f32, ulp=want64.abs().max().item() * 2.0 ** -23)
    return _REF[layer, shape]


@pytest.mark.parametrize("loose", [1.0, 6.5])
@pytest.mark.parametrize("shape,nseg", CASES)
def test_conv5_zmarch_split_f16_is_fp32_class(shape, nseg, loose, ops, monkeypatch):
    """conv5 on the z-march: error against float64 <= 1.5x the fp32 error + 1 ulp (with and without ReLU, exact and x6.5 loose input
    bound), out_bound == the exact maximum magnitude stored, two runs bit-equal (the two partial sums of the K split are added in the
    order of the rounds).  nseg: that many z segments per column (CDS_ZMG_NSEG).  Printed, not asserted: the distance to the tiled
    kernel."""
    if not ops.USE_SPLIT_F16:
        pytest.skip("CDS_SPLIT_F16=0: the split-f16 convolution entry is switched off")
    assert ops.conv3d_sf16_supported(CIN, COUT, 2)
    c = _case("conv5", shape, ops)
    D, H, W = shape
    in_bound = (c["x_cl"].abs().amax() * loose).reshape(1)

    def run(deep, relu, ob=None):
        monkeypatch.setenv("CDS_ZMG_DEEP", str(deep))
        if nseg and deep:
            monkeypatch.setenv("CDS_ZMG_NSEG", str(nseg))
        else:
            monkeypatch.delenv("CDS_ZMG_NSEG", raising=False)
        return ops.conv3d_sbf(c["x_cl"], c["wh"], c["b"], COUT, stride=2, relu=relu, in_bound=in_bound, w_inv_scale=c["w_inv"], out_bound=ob)

    for relu in (False, True):
        out_bound = torch.zeros(1, device=DEV)
        got = run(2, relu, out_bound)
        again = run(2, relu)
        tiled = run(0, relu)
        torch.cuda.synchronize()
        assert tuple(got.shape) == ((D - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1, COUT)
        assert float(out_bound) == float(got.abs().max()), (relu, float(out_bound), float(got.abs().max()))
        assert torch.equal(got, again), "two runs of the z-march differ"
        ref64 = c["want64"].clamp_min(0) if relu else c["want64"]
        err = (got.cpu().permute(3, 0, 1, 2).double() - ref64).abs().max().item()
        err_t = (tiled.cpu().permute(3, 0, 1, 2).double() - ref64).abs().max().item()
        print(f"conv5 {D}x{H}x{W} nseg {nseg} bound x{loose} relu {int(relu)}: max err vs float64: z-march {err:.2e}, tiled {err_t:.2e}, "
              f"fp32 {c['err_f32']:.2e}; max |z-march - tiled| {(got - tiled).abs().max().item():.2e}")
        assert err <= 1.5 * c["err_f32"] + c["ulp"], (relu, err, c["err_f32"])


@pytest.mark.parametrize("loose", [1.0, 6.5])
@pytest.mark.parametrize("shape,nseg", CASES2)
def test_conv2_zmarch_no_k_split_is_fp32_class(shape, nseg, loose, ops, monkeypatch):
    """conv2 with both 8-channel rounds in one wave (no exchange through LDS) on the 32-byte ring: the same bar as conv5 above.  The
    split-f16 entry has no tiled kernel for this shape, so there is no distance to print."""
    if not ops.USE_SPLIT_F16:
        pytest.skip("CDS_SPLIT_F16=0: the split-f16 convolution entry is switched off")
    assert ops.conv3d_sf16_supported(16, 16, 1)
    c = _case("conv2", shape, ops)
    D, H, W = shape
    in_bound = (c["x_cl"].abs().amax() * loose).reshape(1)
    if nseg:
        monkeypatch.setenv("CDS_ZMG_NSEG", str(nseg))
    else:
        monkeypatch.delenv("CDS_ZMG_NSEG", raising=False)

    def run(relu, ob=None):
        return ops.conv3d_sbf(c["x_cl"], c["wh"], c["b"], 16, stride=1, relu=relu, in_bound=in_bound, w_inv_scale=c["w_inv"], out_bound=ob)

    for relu in (False, True):
        out_bound = torch.zeros(1, device=DEV)
        got = run(relu, out_bound)
        again = run(relu)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (D, H, W, 16)
        assert float(out_bound) == float(got.abs().max()), (relu, float(out_bound), float(got.abs().max()))
        assert torch.equal(got, again), "two runs of the z-march differ"
        ref64 = c["want64"].clamp_min(0) if relu else c["want64"]
        err = (got.cpu().permute(3, 0, 1, 2).double() - ref64).abs().max().item()
        print(f"conv2 {D}x{H}x{W} nseg {nseg} bound x{loose} relu {int(relu)}: max err vs float64: z-march {err:.2e}, fp32 {c['err_f32']:.2e}")
        assert err <= 1.5 * c["err_f32"] + c["ulp"], (relu, err, c["err_f32"])


def test_conv5_zmarch_auto_keeps_small_volumes_tiled(ops, monkeypatch):
    """CDS_ZMG_DEEP=1 (the default) sends a volume of a handful of columns to the tiled kernel: bit-equal to CDS_ZMG_DEEP=0."""
    if not ops.USE_SPLIT_F16:
        pytest.skip("CDS_SPLIT_F16=0: the split-f16 convolution entry is switched off")
    g = torch.Generator().manual_seed(7)
    x_cl = torch.randn(8, 16, 32, CIN, generator=g).to(DEV)
    w = torch.randn(COUT, CIN, 3, 3, 3, generator=g) / (27 * CIN) ** 0.5
    wh, w_inv = ops.split_pack_conv3d(w.to(DEV), f16=True)
    in_bound = x_cl.abs().amax().reshape(1)
    monkeypatch.delenv("CDS_ZMG_NSEG", raising=False)
    outs = []
    for deep in ("0", "1"):
        monkeypatch.setenv("CDS_ZMG_DEEP", deep)
        outs.append(ops.conv3d_sbf(x_cl, wh, None, COUT, stride=2, relu=True, in_bound=in_bound, w_inv_scale=w_inv))
    assert torch.equal(outs[0], outs[1])
