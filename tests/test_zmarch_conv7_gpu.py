"""conv7 of CostRegNet (ConvTranspose3d 64 -> 32, k3 s2 p1 op1, + BN shift, ReLU, residual) on the z-marching class-per-wave kernel in
split-f16 arithmetic (csrc/deconv3d_zm.hip: deconv3d_zm64_kernel), forced with CDS_DZM_DEEP=2 whatever the volume's size.  The bar is
that of the project's other split-f16 layers: against a float64 transposed convolution evaluated by PyTorch on the CPU no worse than
1.5x the fp32 evaluation of the same expression + one ulp of the result scale."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CIN, COUT = 64, 32

# input cells (D, H, W): the first four cut the 16 x 4 column by one cell in x and y and leave a partial last tile; then forced z
# segments (CDS_DZM_NSEG); then the M1 volume itself (level 3 of 192 x 512 x 640), once
CASES = [((3, 5, 17), None), ((5, 9, 20), None), ((4, 6, 33), None), ((6, 11, 37), None), ((21, 13, 40), 4), ((9, 13, 70), 3)]
M1 = (24, 64, 80)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cds_mvsnet_amd import ops as o
    assert o.version() >= 100
    return o


def _check(ops, monkeypatch, shape, nseg, loose, variants):
    D, H, W = shape
    g = torch.Generator().manual_seed(7000 + D * 100 + W)
    x = torch.randn(CIN, D, H, W, generator=g) * torch.exp(torch.randn(CIN, 1, 1, 1, generator=g))     # uneven channel scales
    w = torch.randn(CIN, COUT, 3, 3, 3, generator=g) / (27 * CIN / 8) ** 0.5
    b = torch.randn(COUT, generator=g)
    want64 = F.conv_transpose3d(x.double().unsqueeze(0), w.double(), b.double(), stride=2, padding=1, output_padding=1)[0]
    want32 = F.conv_transpose3d(x.unsqueeze(0), w, b, stride=2, padding=1, output_padding=1)[0]
    skip = torch.randn(want32.shape, generator=g)
    wpk = w.permute(0, 2, 3, 4, 1).reshape(CIN, 27, COUT).contiguous().to(DEV)
    chain32 = ops.deconv3d_k3s2(x.to(DEV), wpk, b.to(DEV), relu=False).cpu()
    x_cl = x.permute(1, 2, 3, 0).contiguous().to(DEV)
    skip_cl = skip.permute(1, 2, 3, 0).contiguous().to(DEV)
    in_bound = (x_cl.abs().amax() * loose).reshape(1)
    wh, w_inv = ops.split_pack_deconv3d(w.to(DEV), f16=True)

    def run(deep, relu, sk, ob=None):
        monkeypatch.setenv("CDS_DZM_DEEP", str(deep))
        if nseg and deep:
            monkeypatch.setenv("CDS_DZM_NSEG", str(nseg))
        else:
            monkeypatch.delenv("CDS_DZM_NSEG", raising=False)
        return ops.deconv3d_sbf(x_cl, wh, b.to(DEV), COUT, relu=relu, skip=skip_cl if sk else None, in_bound=in_bound, w_inv_scale=w_inv,
                                out_bound=ob)

    for relu, sk in variants:
        out_bound = torch.zeros(1, device=DEV)
        got = run(2, relu, sk, out_bound)
        again = run(2, relu, sk)
        tiled = run(0, relu, sk)
        torch.cuda.synchronize()
        assert float(out_bound) == float(got.abs().max()), (relu, sk, float(out_bound), float(got.abs().max()))
        assert torch.equal(got, again), "two runs of the z-march differ"

        def expr(v, s):   # the layer's expression on a convolution result v, in v's precision
            v = v.clamp_min(0) if relu else v
            return s + v if sk else v
        ref64 = expr(want64, skip.double())
        err_f32 = max((expr(want32, skip).double() - ref64).abs().max().item(), (expr(chain32, skip).double() - ref64).abs().max().item())
        ulp = ref64.abs().max().item() * 2.0 ** -23
        err = (got.cpu().permute(3, 0, 1, 2).double() - ref64).abs().max().item()
        err_t = (tiled.cpu().permute(3, 0, 1, 2).double() - ref64).abs().max().item()
        print(f"deconv3d 64->32 {D}x{H}x{W} nseg {nseg} bound x{loose} relu {int(relu)} skip {int(sk)}: max err vs float64: z-march {err:.2e}, "
              f"tiled {err_t:.2e}, fp32 {err_f32:.2e}; max |z-march - tiled| {(got - tiled).abs().max().item():.2e}")
        assert err <= 1.5 * err_f32 + ulp, (relu, sk, err, err_f32, ulp)


@pytest.mark.parametrize("loose", [1.0, 6.5])
@pytest.mark.parametrize("shape,nseg", CASES)
def test_conv7_zmarch_split_f16_is_fp32_class(shape, nseg, loose, ops, monkeypatch):
    """Error against float64 <= 1.5x the fp32 error + 1 ulp with and without residual and ReLU, with an exact and a loose input bound;
    out_bound == the exact maximum magnitude stored; two runs bit-equal.  Printed, not asserted: the distance to the tiled kernel."""
    if not ops.USE_SPLIT_F16:
        pytest.skip("CDS_SPLIT_F16=0: the split-f16 entries are switched off")
    _check(ops, monkeypatch, shape, nseg, loose, [(False, False), (True, False), (False, True), (True, True)])


def test_conv7_zmarch_m1_volume(ops, monkeypatch):
    """The M1 volume (24 x 64 x 80 cells -> 48 x 128 x 160 x 32) as the network runs it: ReLU, residual, automatic z segments."""
    if not ops.USE_SPLIT_F16:
        pytest.skip("CDS_SPLIT_F16=0: the split-f16 entries are switched off")
    _check(ops, monkeypatch, M1, None, 1.0, [(True, True)])


def test_conv7_zmarch_auto_keeps_small_volumes_tiled(ops, monkeypatch):
    """CDS_DZM_DEEP=1 (the default) and no setting at all send a volume of four columns to the tiled kernel: bit-equal to CDS_DZM_DEEP=0."""
    if not ops.USE_SPLIT_F16:
        pytest.skip("CDS_SPLIT_F16=0: the split-f16 entries are switched off")
    g = torch.Generator().manual_seed(5)
    x_cl = torch.randn(4, 8, 32, CIN, generator=g).to(DEV)
    skip_cl = torch.randn(8, 16, 64, COUT, generator=g).to(DEV)
    w = torch.randn(CIN, COUT, 3, 3, 3, generator=g) / (27 * CIN / 8) ** 0.5
    wh, w_inv = ops.split_pack_deconv3d(w.to(DEV), f16=True)
    in_bound = x_cl.abs().amax().reshape(1)
    outs = []
    for deep in ("0", "1", None):
        if deep is None:
            monkeypatch.delenv("CDS_DZM_DEEP", raising=False)
        else:
            monkeypatch.setenv("CDS_DZM_DEEP", deep)
        outs.append(ops.deconv3d_sbf(x_cl, wh, None, COUT, relu=True, skip=skip_cl, in_bound=in_bound, w_inv_scale=w_inv))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
