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
