"""The fused CostRegNet tail with prob on the matrix cores (csrc/deconv_prob_zm.hip, cds_deconv_prob_zm_sf16_mfma_f32).

Reference: conv_transpose3d with the folded BN -> ReLU -> + skip -> conv3d in torch float64 on the CPU.  The bar is the one of the
split-f16 layers: max error <= 1.5 x the float64 error of the same chain evaluated in plain fp32, at unit-scale outputs.
Shapes (input cells): (a) D3 H7 W31: a 60-wide column seam and a ragged 2-wide column in x, a 12 + 2 split in y, a z seam with
CDS_DPZ_NSEG=2, every column on the border; (b) D4 H19 W91: a fully interior column, all three plane rotations wrapping, the x tile
seams of the prob waves away from any border.
Measured on the MI355X (max error vs float64, new form / VALU form / torch fp32): see profiles/tail_prob_mfma.md."""
import contextlib
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SHAPES = {"a": (3, 7, 31), "b": (4, 19, 91)}


@functools.lru_cache(maxsize=None)
def _case(name, outliers=False):
    """Seeded inputs of one shape and the float64 / fp32 CPU results of the chain (computed once, shared, never modified)."""
    D, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(D * 1000 + H * 10 + W)
    x = torch.randn(16, D, H, W, generator=g) * torch.exp(0.5 * torch.randn(16, 1, 1, 1, generator=g))
    skip = torch.randn(8, 2 * D, 2 * H, 2 * W, generator=g)
    w11 = torch.randn(16, 8, 3, 3, 3, generator=g) / (27 * 2) ** 0.5
    b11 = torch.randn(8, generator=g)
    wp = torch.randn(1, 8, 3, 3, 3, generator=g) / 27 ** 0.5
    spikes = torch.zeros(skip.shape, dtype=torch.bool)
    if outliers:                                     # 0.1 % of the skip voxels at 10^3 x the bulk and one at 10^4 x
        spikes = torch.rand(skip.shape, generator=g) < 1e-3
        skip[spikes] *= 1e3
        one = skip.numel() // 3
        spikes.view(-1)[one] = True
        skip.view(-1)[one] = 1e4

    def chain(dt):
        y = F.conv_transpose3d(x.to(dt)[None], w11.to(dt), b11.to(dt), stride=2, padding=1, output_padding=1).clamp_min(0)
        return F.conv3d(y + skip.to(dt)[None], wp.to(dt), padding=1)[0, 0]

    bulk = ~F.max_pool3d(spikes.any(0)[None, None].float(), 3, 1, 1)[0, 0].bool()      # 3x3x3 window without an outlier
    return {"x": x, "skip": skip, "w11": w11, "b11": b11, "wp": wp, "r64": chain(torch.float64), "r32": chain(torch.float32),
            "bulk": bulk}


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _run(name, nseg, mfma, outliers=False):
    """One launch of the new entry point: prob on the matrix cores, or (knob off) on the VALU in the same library."""
    from cds_mvsnet_amd import ops
    c = _case(name, outliers)
    x_cl = c["x"].permute(1, 2, 3, 0).contiguous().to(DEV)
    skip_cl = c["skip"].permute(1, 2, 3, 0).contiguous().to(DEV)
    wh, winv = ops.split_pack_deconv_prob(c["w11"].to(DEV), f16=True)
    wm, wms = ops.split_pack_prob(c["wp"].to(DEV), f16=True)
    with _env(CDS_DPZ_NSEG=str(nseg) if nseg else None, CDS_DPZ_PROB_MFMA=None if mfma else "0"):
        got = ops.deconv_prob_zm(x_cl, wh, c["b11"].to(DEV), skip_cl, ops.pack_prob_table(c["wp"].to(DEV)),
                                 in_bound=x_cl.abs().amax().reshape(1), w_inv_scale=winv, prob_mfma=wm, prob_inv_scale=wms,
                                 skip_bound=skip_cl.abs().amax().reshape(1), y_gain=ops.deconv_prob_gain(wh, winv))
        torch.cuda.synchronize()
    got = got.cpu()
    assert got.shape == c["r64"].shape and torch.isfinite(got).all()
    return got


def _errors(name, nseg, outliers=False):
    c = _case(name, outliers)
    m = c["bulk"]
    e = lambda t: (t.double() - c["r64"])[m].abs().max().item()
    return e(_run(name, nseg, True, outliers)), e(_run(name, nseg, False, outliers)), e(c["r32"])


CASES = [("a", 0), ("a", 2), ("b", 0)]


@pytest.mark.parametrize("name,nseg", CASES)
def test_prob_on_matrix_cores_is_fp32_class(name, nseg):
    err, err_valu, err32 = _errors(name, nseg)
    print(f"tail prob mfma {name} nseg {nseg}: max err vs float64 {err:.3e} (VALU form {err_valu:.3e}, torch fp32 {err32:.3e})")
    assert err <= 1.5 * err32, (err, err32)
    assert err_valu <= 1.5 * err32, (err_valu, err32)      # the VALU form behind the knob is held to the same bar


@pytest.mark.parametrize("name,nseg", CASES)
def test_prob_on_matrix_cores_against_valu_form(name, nseg):
    """Two different fp32 sums of the same 216 terms: they differ by no more than the sum of their own float64 errors."""
    err, err_valu, _ = _errors(name, nseg)
    diff = (_run(name, nseg, True) - _run(name, nseg, False)).abs().max().item()
    print(f"tail prob mfma {name} nseg {nseg}: max |mfma - valu| {diff:.3e} (own errors {err:.3e} + {err_valu:.3e})")
    assert diff > 0.0, "the knob did not select another form"
    assert diff <= err + err_valu, (diff, err, err_valu)


def test_call_without_the_keywords_derives_the_same_operands():
    """A split-f16 call that brings only in_bound / w_inv_scale runs the same form on derived operands: the same bits."""
    from cds_mvsnet_amd import ops
    c = _case("b")
    x_cl = c["x"].permute(1, 2, 3, 0).contiguous().to(DEV)
    skip_cl = c["skip"].permute(1, 2, 3, 0).contiguous().to(DEV)
    wh, winv = ops.split_pack_deconv_prob(c["w11"].to(DEV), f16=True)
    with _env(CDS_DPZ_NSEG=None, CDS_DPZ_PROB_MFMA=None):
        got = ops.deconv_prob_zm(x_cl, wh, c["b11"].to(DEV), skip_cl, ops.pack_prob_table(c["wp"].to(DEV)),
                                 in_bound=x_cl.abs().amax().reshape(1), w_inv_scale=winv).cpu()
    assert torch.equal(got, _run("b", 0, True))


def test_prob_on_matrix_cores_loose_bound_and_outliers():
    """Shape (a) with 0.1 % of the skip voxels at 10^3 x the bulk and one at 10^4 x: the scale of y's fp16 terms is set by the
    outliers; the outputs whose 3x3x3 window holds none stay fp32-class."""
    c = _case("a", True)
    assert 0.3 < c["bulk"].float().mean().item() < 0.95
    err, err_valu, err32 = _errors("a", 0, True)
    print(f"tail prob mfma outliers: bulk max err vs float64 {err:.3e} (VALU form {err_valu:.3e}, torch fp32 {err32:.3e})")
    assert err <= 1.5 * err32, (err, err32)
