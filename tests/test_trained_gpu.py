"""The HIP inference path - split-f16 by default (csrc/sbf_common.hpp) - on TRAINED weights.

seeded_init_ gives BatchNorm folds of 0.6 - 1.8; the reference's checkpoints fold their CostRegNet weights by up to 90x (running_var
down to 3e-6) and split-f16 scales each folded weight tensor by ONE power of two.  These tests run the model on the trained weights of
tests/golden/g12_trained_*.npz and g13_trained_costreg*.npz against the reference's recorded forward, and every CostRegNet layer on
the trained stage-3 CostRegNet against float64, with the bounds the model passes.  A spy on the library object asserts that the
split-f16 entry points really ran (no test here may pass on another path)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_trained_checkpoints import CKPTS, _trained, trained_costreg, trained_costreg_state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
# the split-f16 inference entry points of the default forward: CostRegNet (conv0 - conv6, conv7, conv9, conv11 + prob) and FeatureNet
# (conv00, the DynamicConvs, the stride-2 downsamples)
SF16_FORWARD = {"cds_conv3d_sf16_f32", "cds_deconv3d_sf16_f32", "cds_deconv3d_zm_sf16_f32", "cds_deconv_prob_zm_sf16_f32",
                "cds_conv00_cl_sf16_f32", "cds_dynconv_cl_sf16_f32", "cds_conv2d_k3s2_cl_sf16_f32"}


class _CallRecorder:
    """Stands in for the loaded library object and records the names of the entry points fetched through it."""

    def __init__(self, lib):
        self._lib, self.names = lib, set()

    def __getattr__(self, name):
        self.names.add(name)
        return getattr(self._lib, name)


def _forward_g12_scene(sd):
    """CDSMVSNet(refine=True) with state dict ``sd`` on the G12 scene (3 views, 192x128, seed 4, T = 0.01) on the GPU; the names of
    the library entry points it called."""
    from cds_mvsnet_amd import CDSMVSNet, _lib, ops, synth
    assert ops.USE_SPLIT_F16, "CDS_SPLIT_F16=0: these tests are about the split-f16 default"
    model = CDSMVSNet(refine=True, depth_interals_ratio=(4.0, 1.5, 0.75))
    model.load_state_dict(sd, strict=True)
    model = model.eval().to(DEV)
    N, H, W = 3, 128, 192
    imgs = synth.make_images(N, H, W, seed=4).to(DEV)
    cams = {k: v.to(DEV) for k, v in synth.make_cameras(N, H, W, refine=True, seed=4).items()}
    dv = synth.make_depth_values().to(DEV)
    rec = _CallRecorder(_lib.load())
    old = _lib._lib
    _lib._lib = rec
    try:
        with torch.no_grad():
            out = model(imgs, cams, dv, temperature=0.01)
        torch.cuda.synchronize()
    finally:
        _lib._lib = old
    return out, rec.names


def _check_against_reference(out, want, tag):
    """The bars test_full_forward holds against G6: stage depth / confidence mean <= 1e-3, norm_curv max <= 1e-4, refined mean <= 1e-3."""
    for k in ("stage1", "stage2", "stage3"):
        st = out[k]
        for key in ("depth", "photometric_confidence", "norm_curv"):
            assert torch.isfinite(st[key]).all(), (tag, k, key)
        l1 = (st["depth"].cpu() - want[k]["depth"]).abs().mean().item()
        cf = (st["photometric_confidence"].cpu() - want[k]["photometric_confidence"]).abs().mean().item()
        nc = (st["norm_curv"].cpu() - want[k]["norm_curv"]).abs().max().item()
        print(f"{tag} {k}: depth mean-L1 {l1:.2e}, confidence mean {cf:.2e}, norm_curv max {nc:.2e}")
        assert l1 <= 1e-3 and cf <= 1e-3 and nc <= 1e-4, (tag, k, l1, cf, nc)
    assert torch.isfinite(out["refined_depth"]).all()
    rl1 = (out["refined_depth"].cpu() - want["refined_depth"]).abs().mean().item()
    print(f"{tag} refined depth mean-L1 {rl1:.2e}")
    assert rl1 <= 1e-3, (tag, rl1)


@pytest.mark.parametrize("path", CKPTS)
def test_hip_forward_on_trained_checkpoint(path, seeded_state):
    """G12 on the GPU: the trained FeatureNet / visibility / refinement weights (seeded CostRegNets) through the default split-f16
    forward against the reference's recorded outputs."""
    sd, want, _ = _trained(path, seeded_state(True).state_dict())
    assert len(sd) == 387
    out, names = _forward_g12_scene(sd)
    assert SF16_FORWARD <= names, SF16_FORWARD - names
    _check_against_reference(out, want, path.split("/")[0])


def test_hip_forward_with_trained_costreg(seeded_state):
    """G13 on the GPU: as above with the TRAINED stage-3 CostRegNet (BatchNorm folds up to 90x)."""
    sd, want = trained_costreg_state(seeded_state(True).state_dict())
    assert len(sd) == 387
    out, names = _forward_g12_scene(sd)
    assert SF16_FORWARD <= names, SF16_FORWARD - names
    _check_against_reference(out, want, "g13")


# -------------------------------------------------------------------------------------------------------------------------------------
# the trained stage-3 CostRegNet layer by layer
# -------------------------------------------------------------------------------------------------------------------------------------
LAYERS = ("conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11")


def _spy_layers(monkeypatch, ops):
    """Patch the four split-f16 CostRegNet wrappers of ops; -> the list that receives one record per call (in network order)."""
    seen = []

    def wrap(name):
        orig = getattr(ops, name)

        def spy(x_cl, wsplit, *args, **kw):
            ib = kw.get("in_bound")
            assert ib is not None, (name, "called without a bound: not the split-f16 form")
            in_bound = float(ib)                       # the producer's published max (stream-ordered read)
            out = orig(x_cl, wsplit, *args, **kw)
            torch.cuda.synchronize()
            skip = kw.get("skip")
            if name == "deconv_prob_zm":          # (bias, skip, prob_table, ...)
                skip = args[1]
            ob = kw.get("out_bound")
            seen.append({"fn": name, "x": x_cl, "skip": skip, "in_bound": in_bound, "out": out,
                         "out_bound": float(ob) if ob is not None else None, "w_inv": kw.get("w_inv_scale")})
            return out
        monkeypatch.setattr(ops, name, spy)

    for n in ("conv3d_sbf", "deconv3d_sbf", "deconv3d_zm", "deconv_prob_zm"):
        wrap(n)
    return seen


def _fold(unit):
    """The BN-folded weight and shift of one ConvBn3d exactly as CostRegNet._pack forms them (fp32)."""
    from cds_mvsnet_amd.model import _bn_fold
    scale, shift = _bn_fold(unit.bn)
    w = unit.conv.weight.detach()
    w = w * (scale.view(1, -1, 1, 1, 1) if unit.transposed else scale.view(-1, 1, 1, 1, 1))
    return w, shift


def _layer_ref(net, name, x, skip, dtype):
    """One layer (+ its residual; conv11: + the conv0 residual and prob) on planar [1,C,D,H,W] tensors in ``dtype`` (PyTorch)."""
    unit = getattr(net, name)
    w, b = _fold(unit)
    w, b = w.to(dtype), b.to(dtype)
    if unit.transposed:
        y = F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1).clamp_min(0)
        y = y + skip
        if name == "conv11":
            y = F.conv3d(y, net.prob.weight.detach().to(dtype), None, padding=1)
        return y
    return F.conv3d(x, w, b, stride=unit.conv.stride, padding=1).clamp_min(0)


def _layer_exact(ops, p, name, x, skip):
    """The same layer on the library's exact-fp32 kernels (one fmaf chain per output, planar)."""
    if name in ("conv7", "conv9", "conv11"):
        y = ops.deconv3d_k3s2(x, p[name + ".w"], p[name + ".b"], relu=True, skip=skip)
        return ops.conv3d_k3(y, p["prob.w"], None, relu=False) if name == "conv11" else y
    stride = 2 if name in ("conv1", "conv3", "conv5") else 1
    return ops.conv3d_k3(x, p[name + ".w"], p[name + ".b"], stride=stride, relu=True)


def _planar(t):
    return t.permute(3, 0, 1, 2).contiguous() if t.dim() == 4 else t


def _trained_stage3_volume():
    """(model with the G13 weights, its trained stage-3 CostRegNet, channels-last volume [48,256,320,8], stage_inputs bound): the volume
    from model.stage_net.aggregate on synth features (N = 5) as in test_oracle_parity_large_depth_range."""
    from cds_mvsnet_amd import CDSMVSNet, geometry, ops, seeded_init_, synth
    seeded = seeded_init_(CDSMVSNet(refine=True, ndepths=(48, 32, 8), depth_interals_ratio=(4.0, 1.5, 0.75)), 7).state_dict()
    sd, _ = trained_costreg_state(seeded)
    model = CDSMVSNet(refine=True, depth_interals_ratio=(4.0, 1.5, 0.75))
    model.load_state_dict(sd, strict=True)
    model = model.eval().to(DEV)
    h, w, D, C, N = 256, 320, 48, 8, 5
    feats = synth.make_pair_features(N - 1, C, h, w, seed=31)
    cams = synth.stage_cameras(N, h, w, seed=32)
    hyp = synth.make_hypotheses(D, h, w, seed=33)
    rf = [f["ref"][0][0].to(DEV).contiguous() for f in feats]
    sf = [f["src"][0][0].to(DEV).contiguous() for f in feats]
    ref, src, _, _, bound = ops.stage_inputs(rf, sf, want_bound=True)
    ref_nc = torch.stack([f["ref"][2][0, 0] for f in feats]).to(DEV).contiguous()
    with torch.no_grad():
        vol, _, _, _ = model.stage_net.aggregate(ref, src, ref_nc, geometry.warp_matrices(cams[0]), hyp[0].to(DEV).contiguous(), 2,
                                                 channels_last=True)
    return model, model.cost_regularization[2], vol.contiguous(), bound


def test_trained_costreg_layers_are_fp32_class(monkeypatch):
    """Every split-f16 layer of the trained stage-3 CostRegNet (folds up to 90x) on a real aggregated volume, run with the bound the
    model passes (1: tanh features) and with the stage_inputs bound (max |ref| max |src|): each layer's output against a float64
    evaluation of that layer on the SAME input with the same folded weights within 1.5x the larger of PyTorch's fp32 error and the
    exact-fp32 kernel's (+ one ulp of the output scale); in_bound >= max |input|; the published out_bound = max |output|.  The whole net
    against the float64 oracle: at most 2x the exact-fp32 planar path's error."""
    from cds_mvsnet_amd import model as cm, ops
    from oracle import cds_oracle as O
    name, cr, _ = trained_costreg()
    model, net, vol, si_bound = _trained_stage3_volume()
    p = net._packed.get(net, net._pack)
    assert all(f"{n}.wh" in p for n in LAYERS)
    # float64 oracle and the exact-fp32 planar path on the whole net
    vp = _planar(vol)
    sd64 = {k[len("cost_regularization.2."):]: v.double().to(DEV) for k, v in cr.items() if v.is_floating_point()}
    with torch.no_grad():
        want64 = O.cost_regularization(vp.double()[None], {"n." + k: v for k, v in sd64.items()}, "n")[0, 0]
        exact = net(vp)
    err_exact = (exact.double() - want64).abs().max().item()
    lines = [f"trained stage-3 CostRegNet of {name} (max BN fold {max((cr[k].abs() / torch.sqrt(cr[k[:-6] + 'running_var'] + 1e-5)).max().item() for k in cr if k.endswith('.bn.weight')):.1f}), "
             f"volume {tuple(vol.shape)} max |v| {vol.abs().max().item():.3e}"]
    for tag, bound in (("model bound 1", cm._unit_bound(DEV)), ("stage_inputs bound", si_bound)):
        assert float(bound) >= vol.abs().max().item()
        seen = _spy_layers(monkeypatch, ops)
        with torch.no_grad():
            got = net(vol, channels_last=True, bound=bound)
        torch.cuda.synchronize()
        monkeypatch.undo()
        assert [r["fn"] for r in seen] == ["conv3d_sbf"] * 7 + ["deconv3d_sbf", "deconv3d_zm", "deconv_prob_zm"], [r["fn"] for r in seen]
        assert torch.isfinite(got).all(), tag
        err = (got.double() - want64).abs().max().item()
        lines.append(f"[{tag} = {float(bound):.3e}] whole net vs float64 oracle: split-f16 {err:.3e}, exact-fp32 planar {err_exact:.3e}")
        for lname, r in zip(LAYERS, seen):
            x, out = r["x"], r["out"]
            assert torch.isfinite(out).all(), (tag, lname)
            xmax = x.abs().max().item()
            assert r["in_bound"] >= xmax, (tag, lname, r["in_bound"], xmax)
            if r["out_bound"] is not None:
                assert r["out_bound"] == out.abs().max().item(), (tag, lname, r["out_bound"], out.abs().max().item())
            xp = _planar(x)[None]
            sp = _planar(r["skip"])[None] if r["skip"] is not None else None
            with torch.no_grad():
                r64 = _layer_ref(net, lname, xp.double(), sp.double() if sp is not None else None, torch.float64)[0]
                r32 = _layer_ref(net, lname, xp, sp, torch.float32)[0]
                e32 = _layer_exact(ops, p, lname, xp[0], sp[0] if sp is not None else None)
            gotp = _planar(out) if out.dim() == 4 else out[None]
            assert gotp.shape == r64.shape, (lname, gotp.shape, r64.shape)
            e = (gotp.double() - r64).abs().max().item()
            ef = max((r32.double() - r64).abs().max().item(), (e32.double() - r64).abs().max().item())
            ulp = r64.abs().max().item() * 2.0 ** -23
            lines.append(f"[{tag}] {lname:6s} in_bound {r['in_bound']:.3e} max|x| {xmax:.3e} out max {out.abs().max().item():.3e}: "
                         f"split-f16 {e:.3e}, fp32 {ef:.3e} (torch {(r32.double() - r64).abs().max().item():.3e}, "
                         f"exact kernel {(e32.double() - r64).abs().max().item():.3e}), ratio {e / ef if ef else float('inf'):.2f}")
            assert np.isfinite(e) and e <= 1.5 * ef + ulp, (tag, lname, e, ef)
        assert err <= 2.0 * err_exact, (tag, err, err_exact)
    print("\n" + "\n".join(lines))
