"""The split-f16 conv-arithmetic mode of the CostRegNet training convolutions (train_ops.conv_arithmetic("split_f16"),
csrc/train3d_sf16.hip) on the MI355X: every layer shape and pass against float64, the device-resident bounds, the whole network,
the training step eager / captured / with the side stream, and that the default never touches the new entry points."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")

# every (Cin, Cout, stride, transposed) of CostRegNet(C, 8) for C in {8, 16, 32} (prob 8 -> 1 stays fp32)
LAYERS = sorted({(c, 8, 1, False) for c in (8, 16, 32)} | {(8, 16, 2, False), (16, 16, 1, False), (16, 32, 2, False),
                                                          (32, 32, 1, False), (32, 64, 2, False), (64, 64, 1, False),
                                                          (64, 32, 2, True), (32, 16, 2, True), (16, 8, 2, True)})
VOLUMES = [(8, 24, 40), (16, 40, 56), (6, 10, 40)]     # the last: tails along y and z of every tile


def _ref(x, w, stride, transposed):
    return F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1) if transposed else F.conv3d(x, w, stride=stride, padding=1)


def _layer_case(cin, cout, stride, transposed, vol, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    D, H, W = vol
    if transposed:
        D, H, W = D // 2, H // 2, W // 2                    # the volume is the layer's output
    x = torch.randn(B, cin, D, H, W, generator=g) * torch.exp(torch.randn(1, cin, 1, 1, 1, generator=g))   # uneven channel scales
    w = torch.randn(*((cin, cout) if transposed else (cout, cin)), 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    return x, w


def _torch_passes(x, w, gout, stride, transposed, dtype):
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    wr = w.detach().to(dtype).clone().requires_grad_(True)
    y = _ref(xr, wr, stride, transposed)
    y.backward(gout.to(dtype))
    return y.detach(), xr.grad, wr.grad


def _hip_passes(x, w, gout, stride, transposed, x_bound=None, dy_bound=None, mode="split_f16"):
    from cds_mvsnet_amd import train_ops
    xd = x.detach().to(DEV).requires_grad_(True)
    wd = w.detach().to(DEV).requires_grad_(True)
    with train_ops.conv_arithmetic(mode):
        y = train_ops.Conv3dK3.apply(xd, wd, stride, transposed, x_bound, dy_bound)
    y.backward(gout.to(DEV))
    torch.cuda.synchronize()
    return y.detach().cpu(), xd.grad.cpu(), wd.grad.cpu()


def _check(name, got, r64, r32, mask=None, f32=None):
    """err(got) <= 1.5 x the fp32 error + one ulp; the fp32 error: PyTorch's fp32 evaluation and, when given, the library's own fp32
    mode (test_conv3d_split_f16_is_fp32_class takes the larger of PyTorch's and the fp32 kernel chain's in the same way)."""
    if mask is not None:
        got, r64, r32 = got[mask], r64[mask], r32[mask]
        f32 = f32[mask] if f32 is not None else None
    err = (got.double() - r64).abs().max().item()
    err32 = (r32.double() - r64).abs().max().item()
    if f32 is not None:
        err32 = max(err32, (f32.double() - r64).abs().max().item())
    ulp = r64.abs().max().item() * 2.0 ** -23
    assert np.isfinite(err) and err <= 1.5 * err32 + ulp, (name, err, err32)
    return err, err32


@pytest.mark.parametrize("vol", VOLUMES)
@pytest.mark.parametrize("cin,cout,stride,transposed", LAYERS)
def test_layer_passes_are_fp32_class(cin, cout, stride, transposed, vol):
    """Forward, data gradient and weight gradient of one layer against float64 (CPU): no worse than 1.5 x PyTorch's own fp32 (+ one
    ulp of the result scale) - the bar of test_conv3d_split_f16_is_fp32_class; bounds measured on the device (absmax kernel)."""
    x, w = _layer_case(cin, cout, stride, transposed, vol, seed=cin * 1000 + cout * 10 + stride + vol[0])
    y64 = _ref(x.double(), w.double(), stride, transposed)
    gout = torch.randn(y64.shape, generator=torch.Generator().manual_seed(5)) * 1e-3
    r64 = _torch_passes(x, w, gout, stride, transposed, torch.float64)
    r32 = _torch_passes(x, w, gout, stride, transposed, torch.float32)
    got = _hip_passes(x, w, gout, stride, transposed)
    f32 = _hip_passes(x, w, gout, stride, transposed, mode="f32")
    for name, a, b, c, d in zip(("y", "dx", "dw"), got, r64, r32, f32):
        assert a.shape == b.shape, (name, a.shape, b.shape)
        err, err32 = _check(name, a, b, c, f32=d)
        print(f"{cin}->{cout} s{stride}{'T' if transposed else ''} {vol} {name}: split-f16 {err:.2e} fp32 {err32:.2e}")


@pytest.mark.parametrize("cin,cout,stride,transposed", [(16, 16, 1, False), (16, 32, 2, False), (32, 16, 2, True)])
def test_loose_bounds_keep_the_bar(cin, cout, stride, transposed):
    """A bound 2^8 above the true maximum (of x and of the output gradient) only moves the tensor scale: the bar still holds."""
    x, w = _layer_case(cin, cout, stride, transposed, VOLUMES[0], seed=11)
    y64 = _ref(x.double(), w.double(), stride, transposed)
    gout = torch.randn(y64.shape, generator=torch.Generator().manual_seed(6))
    r64 = _torch_passes(x, w, gout, stride, transposed, torch.float64)
    r32 = _torch_passes(x, w, gout, stride, transposed, torch.float32)
    xb = (x.abs().max() * 256).reshape(1).to(DEV)
    gb = (gout.abs().max() * 256).reshape(1).to(DEV)
    got = _hip_passes(x, w, gout, stride, transposed, x_bound=xb, dy_bound=gb)
    f32 = _hip_passes(x, w, gout, stride, transposed, mode="f32")
    for name, a, b, c, d in zip(("y", "dx", "dw"), got, r64, r32, f32):
        _check(name, a, b, c, f32=d)


def test_published_bounds_are_exact():
    """The BatchNorm forward publishes max |out| (skip included), its backward max |dy|, the absmax kernel max |x|: exactly."""
    from cds_mvsnet_amd import train_ops
    g = torch.Generator().manual_seed(3)
    # V % 4 == 0: the float4 loops of the BatchNorm passes; V = 6 and 105: their scalar loops (CostRegNet's deepest level is 1 x 2 x 3)
    for B, C, D, H, W in ((2, 16, 8, 12, 20), (2, 64, 1, 2, 3), (1, 8, 3, 5, 7)):
        y = (torch.randn(B, C, D, H, W, generator=g) * 3).to(DEV)
        skip = torch.randn(B, C, D, H, W, generator=g).to(DEV)
        gamma = torch.rand(C, generator=g).to(DEV) + 0.5
        beta = torch.randn(C, generator=g).to(DEV)
        dout = torch.randn(B, C, D, H, W, generator=g).to(DEV)
        for sk in (None, skip):
            ob, db = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
            yy = y.clone().requires_grad_(True)
            out = train_ops.BnRelu3d.apply(yy, gamma, beta, sk, None, None, 0.1, 1e-5, True, ob, db)
            out.backward(dout)
            torch.cuda.synchronize()
            assert float(ob) == float(out.detach().abs().max()), (B, C, D, H, W)
            assert float(db) == float(yy.grad.abs().max()), (B, C, D, H, W)
    for n in (1, 7, 4096, 1 << 20):
        x = torch.randn(n, generator=g).to(DEV)
        assert float(train_ops.absmax_bound(x)) == float(x.abs().max())


def test_whole_network_bounds_cover_their_tensors():
    """Inside cost_regularization every bound a convolution receives is >= max |its operand| (forward input and output gradient)."""
    from cds_mvsnet_amd import CostRegNet, seeded_init_, train_ops
    net = seeded_init_(CostRegNet(16, 8), 3).train().to(DEV)
    seen = []
    orig = train_ops.conv3d_sf16

    def spy(x, pack, winv, x_bound, cout, mode):
        seen.append((x.detach().abs().max(), x_bound))
        return orig(x, pack, winv, x_bound, cout, mode)

    train_ops.conv3d_sf16 = spy
    try:
        x = torch.randn(2, 16, 8, 16, 24, device=DEV, requires_grad=True)
        with train_ops.conv_arithmetic("split_f16"):
            y = train_ops.cost_regularization(net, x)
        y.backward(torch.randn_like(y))
        torch.cuda.synchronize()
    finally:
        train_ops.conv3d_sf16 = orig
    assert len(seen) == 20                                   # 10 layers: forward and data gradient
    for m, b in seen:
        assert float(b) >= float(m) > 0


def test_zero_gradient_gives_exact_zeros():
    for cin, cout, stride, tr in ((16, 16, 1, False), (16, 32, 2, False), (32, 16, 2, True)):
        x, w = _layer_case(cin, cout, stride, tr, VOLUMES[0], seed=2)
        yshape = _ref(x, w, stride, tr).shape
        _, dx, dw = _hip_passes(x, w, torch.zeros(yshape), stride, tr)
        assert torch.isfinite(dx).all() and torch.isfinite(dw).all()
        assert (dx == 0).all() and (dw == 0).all()


@pytest.mark.parametrize("kind", ["sparse_1e3", "spike_1e4"])
def test_outlier_gradients_keep_the_bulk_fp32_class(kind):
    """A gradient with 0.1 % of its entries at 10^3 x the bulk, or a single 10^4 x spike: the tensor scale follows the outliers,
    the bulk keeps two fp16 terms of 11 bits each.  Data gradient of a stride-1 layer on the outputs no outlier reaches, and the
    weight gradient as a whole: <= 1.5 x fp32's error (+ one ulp)."""
    cin, cout = 16, 16
    x, w = _layer_case(cin, cout, 1, False, VOLUMES[0], seed=21)
    g = torch.Generator().manual_seed(22)
    gout = torch.randn((2, cout) + tuple(x.shape[2:]), generator=g)
    spikes = torch.zeros_like(gout, dtype=torch.bool)
    if kind == "sparse_1e3":
        spikes = torch.rand(gout.shape, generator=g) < 1e-3
        gout[spikes] *= 1e3
    else:
        spikes.view(-1)[gout.numel() // 3] = True
        gout[spikes] = 1e4
    r64 = _torch_passes(x, w, gout, 1, False, torch.float64)
    r32 = _torch_passes(x, w, gout, 1, False, torch.float32)
    got = _hip_passes(x, w, gout, 1, False)
    f32 = _hip_passes(x, w, gout, 1, False, mode="f32")
    reach = F.max_pool3d(spikes.any(1, keepdim=True).float(), 3, 1, 1).bool().expand_as(r64[1])
    _check("dx bulk", got[1], r64[1], r32[1], mask=~reach, f32=f32[1])
    _check("dw", got[2], r64[2], r32[2], f32=f32[2])


@pytest.mark.parametrize("C,B,D,h,w", [(8, 2, 8, 16, 24), (16, 2, 8, 8, 16), (32, 2, 16, 16, 16)])
def test_costreg_split_f16_vs_torch_autograd(C, B, D, h, w):
    """test_costreg_training_kernels_vs_torch_autograd in the mode: output, input gradient, every parameter gradient, running
    statistics against the float64 PyTorch network, same tolerances.  The middle shape runs with B = 2: at B = 1 its deepest level is
    1 x 1 x 2 voxels, so conv5 / conv6's BatchNorm normalises TWO values whose variance is far below eps - a gradient that amplifies
    any forward rounding difference ~1e5-fold (split-f16 lands 1e-2 from float64 there while every convolution pass of that backward,
    checked one by one against float64, is within fp32's own error: 0.7-3e-7 relative)."""
    from cds_mvsnet_amd import CostRegNet, seeded_init_, train_ops
    import torch_training_ref as TR
    net = seeded_init_(CostRegNet(C, 8), 3).train()
    ref = copy.deepcopy(net).double()
    g = torch.Generator().manual_seed(C + B)
    x = torch.randn(B, C, D, h, w, generator=g)
    gout = torch.randn(B, 1, D, h, w, generator=g)
    xr = x.double().requires_grad_(True)
    yr = TR.cost_regularization(ref, xr)
    yr.backward(gout.double())
    net = net.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    with train_ops.conv_arithmetic("split_f16"):
        yg = train_ops.cost_regularization(net, xg)
    yg.backward(gout.to(DEV))
    scale = yr.abs().max().item()
    assert (yg.detach().cpu().double() - yr.detach()).abs().max().item() < 2e-5 * max(1.0, scale)
    assert (xg.grad.cpu().double() - xr.grad).abs().max().item() < 1e-4 * max(1.0, xr.grad.abs().max().item())
    for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, n
        err = (p.grad.cpu().double() - q.grad).abs().max().item()
        assert err < 5e-4 * max(1e-3, q.grad.abs().max().item()), (n, err, q.grad.abs().max().item())
    for (n, b_), (_, c_) in zip(net.named_buffers(), ref.named_buffers()):
        if b_.dtype.is_floating_point:
            assert (b_.cpu().double() - c_).abs().max().item() < 1e-5 * max(1.0, c_.abs().max().item()), n
        else:
            assert int(b_) == int(c_), n


class _CallRecorder:
    """Stands in for the loaded library object and records the names of the entry points fetched through it."""

    def __init__(self, lib):
        self._lib, self.names = lib, set()

    def __getattr__(self, name):
        self.names.add(name)
        return getattr(self._lib, name)


NEW_SYMBOLS = {"cds_bn3d_norm_bound_f32", "cds_bn3d_bwd_norm_bound_f32", "cds_absmax_bound_f32", "cds_sf16_pack_conv3d_f32",
               "cds_conv3d_k3_sf16_f32", "cds_conv3d_wgrad_sf16_f32"}


def _recorded_step(**kw):
    from cds_mvsnet_amd import CDSMVSNet, _lib, seeded_init_, train as T
    from test_train_harness import _train_sample
    sample = _train_sample(DEV)
    model = seeded_init_(CDSMVSNet(refine=False, ndepths=(48, 32, 8), depth_interals_ratio=(4.0, 2.0, 1.0)), 7).to(DEV)
    opt = T.make_optimizer(model)
    rec = _CallRecorder(_lib.load())
    old = _lib._lib
    _lib._lib = rec
    try:
        loss, dl = T.train_step(model, opt, sample, temperature=0.1, **kw)
    finally:
        _lib._lib = old
    assert np.isfinite(loss) and np.isfinite(dl)
    return rec.names


def test_default_step_calls_no_new_entry_point(monkeypatch):
    from cds_mvsnet_amd import train_ops
    monkeypatch.delenv("CDS_TRAIN_CONV", raising=False)
    assert train_ops.get_conv_arithmetic() == "f32"
    names = _recorded_step()
    assert "cds_conv3d_wgrad_f32" in names and not (names & NEW_SYMBOLS), names & NEW_SYMBOLS
    names = _recorded_step(conv_arithmetic="split_f16")
    assert NEW_SYMBOLS <= names, NEW_SYMBOLS - names


def test_training_step_matches_reference_in_the_mode():
    """The G7 step (tests/golden/g7_training_step.npz) in the mode: every assertion of test_training_step_matches_reference."""
    from cds_mvsnet_amd import train_ops
    import test_hip_parity
    with train_ops.conv_arithmetic("split_f16"):
        test_hip_parity.test_training_step_matches_reference(DEV)


def test_captured_step_equals_eager_steps_in_the_mode():
    """test_captured_train_step_equals_eager_steps (captured vs eager, same bounds) with the mode as the process default."""
    from cds_mvsnet_amd import train_ops
    import test_graphed_gpu
    with train_ops.conv_arithmetic("split_f16"):
        test_graphed_gpu.test_captured_train_step_equals_eager_steps()


def test_switching_the_mode_records_a_new_graph():
    from cds_mvsnet_amd import CDSMVSNet, seeded_init_, train as T, train_ops
    from test_train_harness import _train_sample
    sample = _train_sample(DEV)
    model = seeded_init_(CDSMVSNet(refine=False, ndepths=(48, 32, 8), depth_interals_ratio=(4.0, 2.0, 1.0)), 7).to(DEV)
    opt = T.make_optimizer(model)
    st = T.CapturedTrainStep(model, opt, eager_steps=1)
    losses = []
    for mode in ("f32", "f32", "split_f16", "split_f16", "f32"):
        with train_ops.conv_arithmetic(mode):
            loss, _ = st(sample, 0.1)
            losses.append(float(loss))
    assert st.captures == 2 and len(st._entries) == 2, (st.captures, list(st._entries))
    assert all(np.isfinite(losses)), losses


def test_side_stream_gradients_in_the_mode():
    """test_side_stream_gradients_equal_single_stream_gradients with the mode on: the split-f16 weight gradients stay on the main
    stream, the side stream keeps the fp32 ones; gradient by gradient within the same noise bound."""
    from cds_mvsnet_amd import train_ops
    import test_train_harness
    with train_ops.conv_arithmetic("split_f16"):
        test_train_harness.test_side_stream_gradients_equal_single_stream_gradients()
