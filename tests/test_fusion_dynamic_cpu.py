"""Dynamic-consistency fusion without a GPU: the admission rule on hand-made level tables, the float32
restatement against its float64 twin on the five test scenes, the facts that make those scenes non-trivial, the C ABI
declarations and the host-side argument handling."""
import os
import re

import pytest
import torch

import fusion_dynamic_ref as R
from cds_mvsnet_amd import fusion, infer, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("levels,want", [((2, 2, 11), 2), ((3, 3, 2), 3), ((3, 3, 11), 0), ((1, 11, 11), 0),
                                         ((10,) * 10, 10), ((10,) * 9, 0)])
def test_admission_on_hand_made_levels(levels, want):
    got = R.admit_from_levels(torch.tensor(levels).view(-1, 1), n_min=2, n_max=10)
    assert got.tolist() == [want]


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_reference_fp32_vs_float64(i):
    """Pixels that sit on a threshold flip with rounding; the scenes keep their share well below the GPU tests' caps."""
    a, b = R.case_reference(i, torch.float32), R.case_reference(i, torch.float64)
    lv = (a["levels"] != b["levels"]).float().mean().item()
    mk = (a["mask"] != b["mask"]).float().mean().item()
    print(f"{R.CASE_IDS[i]}: level mismatch {lv:.2e}, mask mismatch {mk:.2e}, kept {a['mask'].mean().item():.3f}, "
          f"levels {sorted(a['levels'].unique().tolist())}")
    assert lv < 1e-3 and mk < 1e-3


def test_scenes_are_not_trivial():
    seven = R.case_reference(2)
    kept = seven["mask"].mean().item()
    at3 = (seven["admit"] == 3).float().mean().item()
    print(f"7 views: kept {kept:.3f}, admitted at n=3 {at3:.4f}")
    assert 0.2 < kept < 0.8
    assert at3 > 0.01                       # the graded levels admit pixels that the tightest level alone does not
    one = R.case_reference(0)               # V = 1 < n_min: nothing is admitted
    assert one["mask"].sum().item() == 0 and one["admit"].sum().item() == 0


def test_new_symbol_is_declared_everywhere():
    from cds_mvsnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "cds_mvsnet_hip.h")).read()
    makefile = open(os.path.join(ROOT, "cds_mvsnet_amd", "csrc", "Makefile")).read()
    name, nargs = "cds_depth_fusion_dynamic_f32", 19
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\);", header, re.M | re.S)
    assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name])
    assert hasattr(_lib.load(), name)
    assert re.search(r"^SRCS\s*=.*\bfusion_dynamic\.hip\b", makefile, re.M)
    assert re.search(r"^%\.o:.*\bfusion_common\.hpp\b", makefile, re.M)
    csrc = os.path.join(ROOT, "cds_mvsnet_amd", "csrc")
    for src in ("fusion.hip", "fusion_dynamic.hip"):
        assert '#include "fusion_common.hpp"' in open(os.path.join(csrc, src)).read(), src


def test_infer_accepts_the_dynamic_flags():
    args = infer.parse_args(["--testpath", "a", "--testlist", "b", "--outdir", "c", "--fuse", "--filter_method", "dynamic",
                             "--dyn_dist_base", "0.5", "--dyn_rel_base", "0.001", "--dyn_views", "3,8", "--conf", "0.1,0.2,0.3"])
    assert args.filter_method == "dynamic" and args.dyn_dist_base == 0.5 and args.dyn_rel_base == 0.001
    assert args.dyn_views == "3,8" and args.conf == "0.1,0.2,0.3"
    dflt = infer.parse_args(["--testpath", "a", "--testlist", "b", "--outdir", "c"])
    assert dflt.filter_method == "normal" and dflt.dyn_dist_base == 0.25 and dflt.dyn_rel_base == 1.0 / 1300.0
    assert dflt.dyn_views == "2,10"
    cli = fusion.parse_args(["--testpath", "a", "--testlist", "b", "--outdir", "c", "--filter_method", "dynamic",
                             "--dyn_views", "2,6"])
    assert cli.filter_method == "dynamic" and cli.dyn_views == (2, 6) and cli.conf == [0.0, 0.0, 0.0]


def test_host_side_refusals():
    sc = synth.make_fusion_scene(3, 16, 24, seed=1)
    with pytest.raises(RuntimeError):       # no CPU fallback
        fusion.fuse_view_dynamic(sc["depths"][0], sc["confs"][0], sc["cams"][0], sc["depths"][1:], sc["confs"][1:],
                                 sc["cams"][1:])
    cams = fusion.camera_chains(sc["cams"][0], sc["cams"][1:])
    args = (sc["depths"][0], sc["confs"][0], sc["depths"][1:], sc["confs"][1:], cams, (0.0, 0.0, 0.0))
    for bad in ((2, 17), (3, 2), (0, 4)):   # checked before any launch: ValueError, not the RuntimeError of a host tensor
        with pytest.raises(ValueError):
            ops.depth_fusion_dynamic(*args, n_views=bad)
    with pytest.raises(ValueError):
        ops.depth_fusion_dynamic(*args, dist_base=0.0)
    with pytest.raises(ValueError):
        ops.depth_fusion_dynamic(sc["depths"][0], sc["confs"][0], sc["depths"][1:], sc["confs"][1:], cams[:1], (0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        fusion.filter_depth("nowhere", "nowhere", "nowhere.ply", method="gipuma")
