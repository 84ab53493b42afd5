"""CostRegNet.forward in its three inference forms -- split-f16 (a bound is given), split-bf16 (none), exact fp32 on planar volumes --
against the ten layers chained by hand through ops.*, on operands the test packs itself from the folded weights.  The kernels are
deterministic (K-split partial sums are added in a fixed order, the bounds are maxima), so the comparison is bit equality: it pins
the wiring (model.costreg_unet), the choice of kernel and operand per layer, the bound chain, and CostRegNet._pack.

Volume [D,h,w,C] = [16,24,40,C]: the three sizes differ, x tiles are partial at every level and the coarsest level has two planes --
the smallest volume in which a swapped axis, skip or stride cannot cancel out."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LAYERS = ("conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cds_mvsnet_amd import ops as o
    assert o.version() >= 100
    return o


@pytest.fixture(scope="module", params=[8, 32])
def case(request):
    """(eval CostRegNet(C, 8), volume [16,24,40,C] channels-last, {layer: (folded weight in the holder's layout, shift)})."""
    from cds_mvsnet_amd import CostRegNet, seeded_init_
    from test_trained_gpu import _fold
    C = request.param
    net = seeded_init_(CostRegNet(C, 8), 40 + C).eval().to(DEV)
    vol = torch.randn(16, 24, 40, C, generator=torch.Generator().manual_seed(C)).to(DEV)
    with torch.no_grad():
        folded = {n: tuple(t.contiguous() for t in _fold(getattr(net, n))) for n in LAYERS}
    return net, vol, folded


def _chain_split(ops, net, vol, folded, bound):
    """The matrix-core form: split-f16 when a bound is given (and the library has the form switched on), else split-bf16."""
    f16 = bound is not None and ops.USE_SPLIT_F16
    packer = {n: ops.split_pack_conv3d for n in LAYERS}
    packer.update(conv0=ops.split_pack_conv3d_pair, conv7=ops.split_pack_deconv3d, conv9=ops.split_pack_deconv_cls,
                  conv11=ops.split_pack_deconv_prob)
    W, inv = {}, {}
    for n in LAYERS:
        W[n], inv[n] = packer[n](folded[n][0], f16=True) if f16 else (packer[n](folded[n][0]), None)
    B = {n: folded[n][1] for n in LAYERS}
    bnd = torch.zeros((16,), dtype=torch.float32, device=DEV)

    def kw(i, n, publish=True):
        """Layer number i scales by the bound layer i - 1 published in its slot (the first by the caller's), and publishes its own."""
        if not f16:
            return {}
        k = {"in_bound": bound if i == 0 else bnd[i - 1:i], "w_inv_scale": inv[n]}
        if publish:
            k["out_bound"] = bnd[i:i + 1]
        return k

    c0 = ops.conv3d_sbf(vol, W["conv0"], B["conv0"], 8, stride=ops.SBF_PAIR, **kw(0, "conv0"))
    c1 = ops.conv3d_sbf(c0, W["conv1"], B["conv1"], 16, stride=2, **kw(1, "conv1"))
    c2 = ops.conv3d_sbf(c1, W["conv2"], B["conv2"], 16, stride=1, **kw(2, "conv2"))
    c3 = ops.conv3d_sbf(c2, W["conv3"], B["conv3"], 32, stride=2, **kw(3, "conv3"))
    c4 = ops.conv3d_sbf(c3, W["conv4"], B["conv4"], 32, stride=1, **kw(4, "conv4"))
    c5 = ops.conv3d_sbf(c4, W["conv5"], B["conv5"], 64, stride=2, **kw(5, "conv5"))
    c6 = ops.conv3d_sbf(c5, W["conv6"], B["conv6"], 64, stride=1, **kw(6, "conv6"))
    u7 = ops.deconv3d_sbf(c6, W["conv7"], B["conv7"], 32, skip=c4, **kw(7, "conv7"))
    u9 = ops.deconv3d_zm(u7, W["conv9"], B["conv9"], skip=c2, **kw(8, "conv9"))
    return ops.deconv_prob_zm(u9, W["conv11"], B["conv11"], c0, ops.pack_prob_table(net.prob.weight), **kw(9, "conv11", publish=False))


def _chain_exact(ops, net, vol, folded):
    """The exact-fp32 planar kernels; the stride-1 layers with 16 | Cin, Cout also hand over the ci-fastest copy of their weights."""
    W, WCL, B = {}, {}, {}
    for n in LAYERS:
        w, B[n] = folded[n]
        w = w.permute(0, 2, 3, 4, 1) if getattr(net, n).transposed else w.permute(1, 2, 3, 4, 0)        # [Cin,3,3,3,Cout]
        W[n] = w.reshape(w.shape[0], 27, w.shape[-1]).contiguous()
        WCL[n] = w.permute(1, 2, 3, 4, 0).reshape(27, w.shape[-1], w.shape[0]).contiguous()
    wp = net.prob.weight.detach().permute(1, 2, 3, 4, 0).reshape(8, 27, 1).contiguous()
    c0 = ops.conv3d_k3(vol.permute(3, 0, 1, 2).contiguous(), W["conv0"], B["conv0"])
    c1 = ops.conv3d_k3(c0, W["conv1"], B["conv1"], stride=2)
    c2 = ops.conv3d_k3(c1, W["conv2"], B["conv2"], wcl=WCL["conv2"])
    c3 = ops.conv3d_k3(c2, W["conv3"], B["conv3"], stride=2)
    c4 = ops.conv3d_k3(c3, W["conv4"], B["conv4"], wcl=WCL["conv4"])
    c5 = ops.conv3d_k3(c4, W["conv5"], B["conv5"], stride=2)
    c6 = ops.conv3d_k3(c5, W["conv6"], B["conv6"], wcl=WCL["conv6"])
    u7 = ops.deconv3d_k3s2(c6, W["conv7"], B["conv7"], skip=c4)
    u9 = ops.deconv3d_k3s2(u7, W["conv9"], B["conv9"], skip=c2)
    u11 = ops.deconv3d_k3s2(u9, W["conv11"], B["conv11"], skip=c0)
    return ops.conv3d_k3(u11, wp, None, relu=False)[0]


@pytest.mark.parametrize("form", ["split_f16", "split_bf16", "exact"])
def test_forward_equals_the_hand_chained_layers(form, case, ops):
    """With CDS_SPLIT_F16=0 the library has no split-f16 entry and a forward with a bound runs split-bf16: so does the hand chain."""
    net, vol, folded = case
    with torch.no_grad():
        if form == "exact":
            got = net(vol.permute(3, 0, 1, 2).contiguous())
            want = _chain_exact(ops, net, vol, folded)
        else:
            bound = vol.abs().amax().reshape(1) if form == "split_f16" else None
            got = net(vol, channels_last=True, bound=bound)
            want = _chain_split(ops, net, vol, folded, bound)
    torch.cuda.synchronize()
    assert got.shape == want.shape == vol.shape[:3]
    assert torch.isfinite(want).all() and want.abs().max() > 0
    assert torch.equal(got, want), (form, (got - want).abs().max().item())
