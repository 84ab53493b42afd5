"""Parity of the CPU oracle against the REFERENCE on its own TRAINED checkpoints.

For each of the three checkpoints the reference ships (`pretrained/*/`, loaded by test.py:180-187's rules: 'module.' prefix stripped)
`tests/golden/g12_trained_<name>.npz` holds the trained weights outside CostRegNet - FeatureNet with its DynamicConv blends, the
visibility network, the refinement network - and the reference's `CDSMVSNet.forward` on a synthetic 3-view 192x128 scene at the
evaluation temperature T = 0.01, refine=True (the checkpoints' own arch args); `make_golden.py g12` writes them from the reference tree.
The three CostRegNets (0.89 M of the 0.98 M parameters; too large to store) are the seeded ones of the `seeded_state` fixture, in the
reference's forward as in the oracle's.
`oracle.cds_oracle.forward` on the same scene must agree to the tolerances of SURVEY §8(c): stage depth mean-L1 <= 1e-3, confidence
<= 1e-3, curvature maps <= 2e-5.  The product's loader reads the weights from a file in the reference's checkpoint layout (arch /
epoch / state_dict / monitor_best / a pickled config object, 'module.' prefix as in the original file)."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CKPTS = ["dtu_only/checkpoint-epoch24.pth", "both_dtu_blended/cds_mvsnet.ckpt", "fine_tuning_on_blended/cds_mvsnet.ckpt"]


class _PickledConfig:
    """Stands in for the reference's pickled ``ConfigParser``: a class the weights-only loader refuses."""

    def __init__(self):
        self.config = {"arch": {"type": "CDSMVSNet"}}


def _trained(path, seeded):
    """-> (state dict, reference outputs, 'module.' prefix in the original file) of one checkpoint; CostRegNet from ``seeded``."""
    z = np.load(os.path.join(GOLDEN, "g12_trained_" + path.split("/")[0] + ".npz"))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}
    sd.update({k: v for k, v in seeded.items() if k.startswith("cost_regularization.")})
    want = {}
    for k in z.files:
        if k.startswith("out."):
            parts = k.split(".")[1:]
            if len(parts) == 1:
                want[parts[0]] = torch.from_numpy(z[k])
            else:
                want.setdefault(parts[0], {})[parts[1]] = torch.from_numpy(z[k])
    return sd, want, bool(z["module_prefix"])


@pytest.mark.parametrize("path", CKPTS)
def test_oracle_equals_reference_on_trained_checkpoint(path, tmp_path, seeded_state):
    from cds_mvsnet_amd import CDSMVSNet, synth
    from cds_mvsnet_amd.infer import load_checkpoint
    from oracle import cds_oracle as O
    torch.set_num_threads(8)
    sd, want, prefixed = _trained(path, seeded_state(True).state_dict())
    assert len(sd) == 387
    # the product's loader accepts a file in the reference's layout (placeholder unpickler) and fills every one of the 387 entries
    ck = os.path.join(tmp_path, os.path.basename(path))
    torch.save({"arch": "CDSMVSNet", "epoch": 1, "state_dict": {("module." if prefixed else "") + k: v for k, v in sd.items()},
                "monitor_best": 0, "config": _PickledConfig()}, ck)
    mine = CDSMVSNet(refine=True, depth_interals_ratio=(4.0, 1.5, 0.75))
    load_checkpoint(mine, ck, trust_pickle=True)
    assert all(torch.equal(v, sd[k]) for k, v in mine.state_dict().items())

    N, H, W = 3, 128, 192
    imgs = synth.make_images(N, H, W, seed=4)
    cams = synth.make_cameras(N, H, W, refine=True, seed=4)
    dv = synth.make_depth_values()
    with torch.no_grad():
        got = O.forward(imgs, cams, dv, sd, refine=True, temperature=0.01, exact=True)
    for k in ("stage1", "stage2", "stage3"):
        assert (got[k]["depth"] - want[k]["depth"]).abs().mean() < 1e-3, (path, k)
        assert (got[k]["photometric_confidence"] - want[k]["photometric_confidence"]).abs().mean() < 1e-3, (path, k)
        assert (got[k]["norm_curv"] - want[k]["norm_curv"]).abs().max() < 2e-5, (path, k)
    assert (got["refined_depth"] - want["refined_depth"]).abs().mean() < 1e-3, path


def trained_costreg():
    """-> (checkpoint name, state-dict entries of the trained stage-3 CostRegNet ``cost_regularization.2.*``, reference outputs) of
    tests/golden/g13_trained_costreg*.npz (``make_golden.py g13``; float32 weights stored byte-shuffled)."""
    z = np.load(os.path.join(GOLDEN, "g13_trained_costreg.npz"))
    cr = {}
    for k in z.files:
        if k.startswith("w."):
            v = z[k]
            if "shape." + k[2:] in z.files:      # uint8 [4, n] byte planes -> float32
                v = np.ascontiguousarray(v.T).view(np.float32).reshape(tuple(z["shape." + k[2:]]))
            cr[k[2:]] = torch.from_numpy(np.array(v))
    o = np.load(os.path.join(GOLDEN, "g13_trained_costreg_out.npz"))
    assert str(o["checkpoint"]) == str(z["checkpoint"])
    want = {}
    for k in o.files:
        if k.startswith("out."):
            parts = k.split(".")[1:]
            if len(parts) == 1:
                want[parts[0]] = torch.from_numpy(o[k])
            else:
                want.setdefault(parts[0], {})[parts[1]] = torch.from_numpy(o[k])
    return str(z["checkpoint"]), cr, want


def trained_costreg_state(seeded):
    """The G13 state dict: its checkpoint's G12 weights, the trained stage-3 CostRegNet, the seeded stage-1 / stage-2 ones."""
    name, cr, want = trained_costreg()
    path = next(p for p in CKPTS if p.split("/")[0] == name)
    sd, _, _ = _trained(path, seeded)
    sd.update(cr)
    return sd, want


def test_trained_costreg_fixture():
    """G13 holds the stage-3 CostRegNet whose BatchNorm folds reach furthest (max |gamma| / sqrt(var + eps) = 90.5, far outside the
    0.6 - 1.8 of seeded_init_): every entry of cost_regularization.2 with its shape, and the fold factor it records."""
    from cds_mvsnet_amd import CDSMVSNet
    name, cr, _ = trained_costreg()
    assert name in [p.split("/")[0] for p in CKPTS]
    want = {k: v.shape for k, v in CDSMVSNet(refine=True).state_dict().items() if k.startswith("cost_regularization.2.")}
    assert {k: v.shape for k, v in cr.items()} == want
    fold = max((cr[k].abs() / torch.sqrt(cr[k[:-6] + "running_var"] + 1e-5)).max().item() for k in cr if k.endswith(".bn.weight"))
    z = np.load(os.path.join(GOLDEN, "g13_trained_costreg.npz"))
    assert fold == pytest.approx(float(z["max_fold"]), rel=1e-6) and fold > 50.0, fold


def test_oracle_equals_reference_with_trained_costreg(seeded_state):
    """G13: the oracle against the reference's forward with a TRAINED CostRegNet at stage 3 (the rest as in G12), same bars."""
    from cds_mvsnet_amd import synth
    from oracle import cds_oracle as O
    torch.set_num_threads(8)
    sd, want = trained_costreg_state(seeded_state(True).state_dict())
    assert len(sd) == 387
    N, H, W = 3, 128, 192
    imgs = synth.make_images(N, H, W, seed=4)
    cams = synth.make_cameras(N, H, W, refine=True, seed=4)
    dv = synth.make_depth_values()
    with torch.no_grad():
        got = O.forward(imgs, cams, dv, sd, refine=True, temperature=0.01, exact=True)
    for k in ("stage1", "stage2", "stage3"):
        assert (got[k]["depth"] - want[k]["depth"]).abs().mean() < 1e-3, k
        assert (got[k]["photometric_confidence"] - want[k]["photometric_confidence"]).abs().mean() < 1e-3, k
        assert (got[k]["norm_curv"] - want[k]["norm_curv"]).abs().max() < 2e-5, k
    assert (got["refined_depth"] - want["refined_depth"]).abs().mean() < 1e-3
