"""tests/train3d_ref.py checked on the CPU: the tap-by-tap weight gradient against float64 autograd, the rounding model of the BatchNorm
kernels against a float32 emulation of their formulas, and the two conditions the GPU file (tests/test_train3d_gpu.py) relies on for
the very cases it runs: no pre-activation within its bar of the ReLU boundary, every integer sum below 2^24."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import train3d_ref as R


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("case", R.WGRAD_CASES + R.WGRAD_TILE_CASES, ids=str)
def test_wgrad_ref_equals_autograd(case):
    """Stride 1, stride 2 with odd and even input extents, partial channel blocks: the convolution role (g = dy, xin = x)."""
    g, xin = R.real_case("wgrad", *case)
    want = R.wgrad_torch(g, xin, case[5], torch.float64)
    assert _rel(R.wgrad_ref(g, xin, case[5]), want) < 1e-12


@pytest.mark.parametrize("cin,cout,vol", [(64, 32, (2, 4, 6)), (32, 16, (6, 10, 18)), (3, 5, (4, 6, 10))])
def test_wgrad_ref_equals_autograd_transposed_role(cin, cout, vol):
    """ConvTranspose3d(k3, s2, p1, op1): its weight gradient [Cin, Cout, 3, 3, 3] is the same sum with g = x and xin = dy."""
    gen = torch.Generator().manual_seed(cin + cout)
    D, H, W = (v // 2 for v in vol)
    x = torch.randn(2, cin, D, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(cin, cout, 3, 3, 3, generator=gen, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1)
    dy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(dy)
    assert _rel(R.wgrad_ref(x, dy, 2), w.grad) < 1e-12


@pytest.mark.parametrize("cin,cout,stride,transposed", [(8, 16, 2, False), (16, 16, 1, False), (16, 8, 2, True), (8, 1, 1, False)])
def test_layer_weight_gradient_is_wgrad_ref(cin, cout, stride, transposed):
    """layer_ref's dw is wgrad_ref of (dy, x) for a convolution and of (x, dy) for a transposed one: the calls Conv3dK3 makes."""
    x, w, gout = R.real_case("layer", cin, cout, stride, transposed, (6, 10, 40))
    _, _, dw = R.layer_ref(x, w, gout, stride, transposed, torch.float64)
    mine = R.wgrad_ref(x, gout, 2) if transposed else R.wgrad_ref(gout, x, stride)
    assert _rel(mine, dw) < 1e-12


def test_exactness_condition_of_every_integer_case():
    """sum |terms| < 2^24 per output element, and the values are the integers the docstring promises."""
    for case in R.WGRAD_CASES + R.WGRAD_TILE_CASES:
        g, xin = R.int_case("wgrad", *case)
        assert g.dtype == torch.float32 and g.abs().max() <= 3 and xin.abs().max() <= 3 and (g == g.round()).all()
        assert R.exact_headroom("wgrad", (g, xin), case[5]) < R.EXACT_LIMIT, case
    for (cin, cout, stride, tr), vol in itertools.product(R.LAYER_CASES, R.LAYER_VOLUMES):
        x, w, gout = R.int_case("layer", cin, cout, stride, tr, vol)
        assert x.abs().max() <= 3 and w.abs().max() <= 2 and gout.abs().max() <= 3 and (w == w.round()).all()
        assert R.exact_headroom("layer", (x, w, gout), stride, tr) < R.EXACT_LIMIT, (cin, cout, stride, tr, vol)


def test_integer_results_are_exact_in_float32():
    """Under the condition PyTorch's own float32 passes already equal float64 bit for bit: the property the GPU tests ask of the kernels."""
    for cin, cout, stride, tr in [(8, 16, 2, False), (16, 8, 2, True), (8, 1, 1, False)]:
        case = R.int_case("layer", cin, cout, stride, tr, (8, 8, 8))
        for a, b in zip(R.layer_ref(*case, stride, tr, torch.float32), R.layer_ref(*case, stride, tr, torch.float64)):
            assert torch.equal(a.double(), b)


@pytest.mark.parametrize("shape", R.all_bn_shapes(), ids=str)
@pytest.mark.parametrize("offset", R.BN_OFFSETS)
def test_relu_boundary_condition_of_every_bn_case(shape, offset):
    c = R.bn_case(shape, offset)
    assert c["y"].dtype == torch.float32 and c["y"].shape == shape
    assert R.relu_boundary_violations(c["y"], c["gamma"], c["beta"]) == 0
    ref = R.bn_ref(c["y"], c["gamma"], c["beta"], None, c["dout"], None, 0.0, R.BN_EPS, True)      # the closed form IS batch_norm
    q = R.bn_closed_form(c["y"], c["gamma"], c["beta"], c["dout"], R.BN_EPS, True)
    scale = ref["pre"].abs().max().item()
    assert (q["pre"] - ref["pre"]).abs().max().item() < 1e-11 * scale
    assert (q["dy"] - ref["dy"]).abs().max().item() < 1e-11 * max(ref["dy"].abs().max().item(), scale)


def test_relu_boundary_condition_fails_far_out():
    """At 1000 sigma the bar outgrows the spacing of the pre-activations: why the channel offsets stop at 30."""
    gen = torch.Generator().manual_seed(1)
    y = torch.randn(2, 16, 8, 12, 20, generator=gen) + 1000.0
    assert R.relu_boundary_violations(y, torch.ones(16), torch.zeros(16)) > 0


@pytest.mark.parametrize("shape", R.BN_SHAPES + [R.BN_ALIGN_SHAPE], ids=str)
@pytest.mark.parametrize("offset", R.BN_OFFSETS)
def test_float32_emulation_stays_within_the_bars(shape, offset):
    """The kernels' formulas with their float32 roundings land inside bn_bars for every output, element by element."""
    c = R.bn_case(shape, offset)
    for relu, use_skip, momentum in itertools.product((True, False), (False, True), R.BN_MOMENTA):
        running = (c["running_mean"], c["running_var"]) if momentum is not None else None
        args = (c["y"], c["gamma"], c["beta"], c["skip"] if use_skip else None, c["dout"], running, momentum or 0.0, R.BN_EPS, relu)
        ref, bars, emu = R.bn_ref(*args), R.bn_bars(*args), R.bn_emulate_f32(*args)
        for name, err, bar, bad in R.bn_compare(emu, ref, bars):
            assert bad == 0, (name, err, bar, bad, relu, use_skip, momentum)


def test_bars_reject_a_bf16_scale():
    c = R.bn_case(R.BN_SHAPES[0], 1.0)
    gamma16 = c["gamma"].bfloat16().float()
    args = (c["y"], c["gamma"], c["beta"], None, c["dout"], None, 0.0, R.BN_EPS, False)
    ref, bars = R.bn_ref(*args), R.bn_bars(*args)
    emu = R.bn_emulate_f32(c["y"], gamma16, *args[2:])
    rows = {name: bad for name, _, _, bad in R.bn_compare(emu, ref, bars)}
    assert rows["out"] > 0 and rows["dy"] > 0
