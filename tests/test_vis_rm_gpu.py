"""GPU tests of the row-marching visibility CNN (csrc/vis_rm.hip, ops.vis_cnn_rm) against the three launches it replaces
(vis_layer1_cl + 2 x conv2d_k3_relu_cl: same fmaf chain, same K-steps and products, same head: the bar is torch.equal) and against a
float64 chain (<= 2e-6, the head bar of test_visibility_layers_channels_last).  Shapes: shorter than the priming depth of the rings,
ragged widths, the seams between the 60-pixel column strips, the seams between row segments (CDS_VIS_NSEG)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

STRIP = 60                       # VR_OWN of csrc/vis_rm.hip

SHAPES = [(1, 1, 1), (1, 2, 5), (2, 3, 16),                                    # shorter than the priming depth
          (1, 8, 33), (4, 20, 36), (3, 13, 100), (6, 37, 50),                  # ragged widths (test_visibility_layers_channels_last)
          (2, 9, 130), (1, 5, STRIP - 1), (1, 5, STRIP), (1, 5, STRIP + 1), (1, 5, 2 * STRIP + 1)]     # strip seams
SEG_SHAPE = (1, 70, 17)
NSEGS = [1, 2, 3, 35]            # 35: segments of two rows, shorter than the three rows a layer looks at


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from cds_mvsnet_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def _case(V, H, W, bias_one):
    """Seeded inputs and weights on the GPU, the three-launch result and the float64 chain (computed once per shape, never modified)."""
    import torch.nn.functional as F
    from cds_mvsnet_amd import ops
    from cds_mvsnet_amd.model import _pack2d
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(V * 100 + W)
    ent, nc = torch.rand(V, H, W, generator=g) * 3.0, torch.rand(V, H, W, generator=g)
    w0, b0 = torch.randn(16, 2, 3, 3, generator=g) / 4.0, torch.randn(16, generator=g) * 0.2
    w1, b1 = torch.randn(16, 16, 3, 3, generator=g) / 12.0, torch.randn(16, generator=g) * 0.2
    w2, b2 = torch.randn(16, 16, 3, 3, generator=g) / 12.0, torch.randn(16, generator=g) * 0.2
    hw, hb = torch.randn(16, generator=g) * 0.3, torch.randn(1, generator=g)
    if bias_one:                 # ReLU(bias) != 0 everywhere: a padding position that holds the convolution instead of zero cannot hide
        b0, b1, b2, hb = torch.ones(16), torch.ones(16), torch.ones(16), torch.ones(1)
    x = torch.stack((ent, nc), 1).double()
    for w, b in ((w0, b0), (w1, b1), (w2, b2)):
        x = F.conv2d(x, w.double(), b.double(), padding=1).clamp_min(0)
    want64 = torch.sigmoid((x * hw.double().view(1, 16, 1, 1)).sum(1) + hb.double())
    args = (ent.to(dev), nc.to(dev), _pack2d(w0.to(dev)), b0.to(dev), ops.split_pack_dynconv([w1.to(dev)]), b1.to(dev),
            ops.split_pack_dynconv([w2.to(dev)]), b2.to(dev), hw.to(dev), hb.to(dev))
    e, n, wp, b0d, ws1, b1d, ws2, b2d, hwd, hbd = args
    x1 = ops.vis_layer1_cl(e, n, wp, b0d)
    x2 = ops.conv2d_k3_relu_cl(x1, ws1, b1d)
    three = ops.conv2d_k3_relu_cl(x2, ws2, b2d, head_w=hwd, head_b=hbd)
    return args, three, want64


def _check(V, H, W, bias_one, ops):
    args, three, want64 = _case(V, H, W, bias_one)
    got = ops.vis_cnn_rm(*args)
    assert tuple(got.shape) == (V, H, W)
    diff = got != three
    err64 = (got.cpu().double() - want64).abs().max().item()
    print(f"vis_cnn_rm {(V, H, W)} bias_one={bias_one}: {int(diff.sum())} of {got.numel()} values differ from the three launches, "
          f"max |fused - float64| = {err64:.3e}")
    assert torch.equal(got, three), (int(diff.sum()), diff.nonzero()[:8].tolist())
    assert err64 <= 2e-6
    return got


@pytest.mark.parametrize("V,H,W", SHAPES)
def test_fused_equals_three_launches(V, H, W, dev, ops, monkeypatch):
    monkeypatch.delenv("CDS_VIS_NSEG", raising=False)
    _check(V, H, W, False, ops)


@pytest.mark.parametrize("nseg", NSEGS)
def test_segment_seams(nseg, dev, ops, monkeypatch):
    """The knob is read per launch: every segment primes its rings with zero rows above 0 / below h and real rows at the inner seams."""
    monkeypatch.setenv("CDS_VIS_NSEG", str(nseg))
    _check(*SEG_SHAPE, False, ops)


@pytest.mark.parametrize("V,H,W,nseg", [(3, 13, 100, 0), (1, 70, 17, 35)])
def test_padding_is_zero_not_relu_of_bias(V, H, W, nseg, dev, ops, monkeypatch):
    """All biases + 1: a layer-1 / layer-2 position outside the image (rows, columns, a segment's priming rows) must hold zero."""
    if nseg:
        monkeypatch.setenv("CDS_VIS_NSEG", str(nseg))
    else:
        monkeypatch.delenv("CDS_VIS_NSEG", raising=False)
    _check(V, H, W, True, ops)


def test_two_calls_equal_bits(dev, ops, monkeypatch):
    monkeypatch.delenv("CDS_VIS_NSEG", raising=False)
    args, _, _ = _case(2, 9, 130, False)
    assert torch.equal(ops.vis_cnn_rm(*args), ops.vis_cnn_rm(*args))


def test_forward_equal_with_knob_on_and_off(dev, monkeypatch):
    """CDSMVSNet on the 320x256, 3-view cascade: every returned tensor equal with the fused kernel and with the three launches."""
    from cds_mvsnet_amd import CDSMVSNet, seeded_init_, synth
    from cds_mvsnet_amd import model as M
    monkeypatch.delenv("CDS_VIS_NSEG", raising=False)
    N, H, W = 3, 256, 320
    model = seeded_init_(CDSMVSNet(refine=False, depth_interals_ratio=(4.0, 1.5, 0.75)), 0).eval().to(dev)
    imgs, cams, dv = synth.make_images(N, H, W, seed=4).to(dev), synth.make_cameras(N, H, W, refine=False, seed=4), synth.make_depth_values()
    calls = []
    real = M.ops.vis_cnn_rm
    monkeypatch.setattr(M.ops, "vis_cnn_rm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    outs = []
    for fused in (True, False):
        monkeypatch.setattr(M, "USE_VIS_FUSED", fused)
        n0 = len(calls)
        with torch.no_grad():
            outs.append(model(imgs, cams, dv, temperature=0.01))
        assert (len(calls) > n0) == fused          # the knob selects the path it names

    def flat(out, pre=""):
        for k in sorted(out):
            if isinstance(out[k], dict):
                yield from flat(out[k], f"{pre}{k}.")
            else:
                yield f"{pre}{k}", out[k]
    a, b = list(flat(outs[0])), list(flat(outs[1]))
    assert [k for k, _ in a] == [k for k, _ in b] and len(a) > 0
    for (k, x), (_, y) in zip(a, b):
        assert torch.equal(x, y), k
