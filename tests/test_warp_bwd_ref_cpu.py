"""tests/warp_bwd_ref.py checked without a GPU: its float64 reference against float64 autograd through F.grid_sample fed the same
positions, its path model on a hand-checkable case, and the preconditions of the cases of tests/test_warp_bwd_gpu.py - which
workgroups of the default K3 backward kernel are boxed, fall back to global atomics or are empty."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_bwd_ref as R  # noqa: E402


def _grid_sample_gradients(i):
    """float64 autograd through F.grid_sample(align_corners=True, padding_mode="zeros") at the reference's positions."""
    V, C, h, w = i["ref"].shape
    pos = R.positions(i["cams"], i["hyp"], V, h, w)
    D = pos[0][0].shape[0]
    ref, src, vis = (i[k].double().clone().requires_grad_(True) for k in ("ref", "src", "vis"))
    vol = 0.0
    for v in range(V):
        gx = pos[v][0].double() / ((w - 1) / 2) - 1
        gy = pos[v][1].double() / ((h - 1) / 2) - 1
        grid = torch.stack((gx, gy), dim=-1).view(1, D * h, w, 2)
        warped = F.grid_sample(src[v:v + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(C, D, h, w)
        vol = vol + vis[v].view(1, 1, h, w) * ref[v].unsqueeze(1) * warped
    (vol * i["G"].double()).sum().backward()
    return ref.grad, src.grad, vis.grad


@pytest.mark.parametrize("name", ["legacy-3x16x4x9x70", "shared-hyp"])
def test_float64_reference_equals_grid_sample_autograd(name):
    """Two small shapes (one with per-pixel, one with shared hypotheses; both with samples that leave the image).  grid_sample gets the
    positions normalised to [-1, 1] and un-normalises them again in float64: its positions differ from the reference's by a few 1e-16 w,
    the gradients by 1e-12 of their scale at most on these white-noise maps."""
    i = R.case_input(name)
    got = R.reference((i["ref"], i["src"]), i["cams"], i["hyp"], i["vis"], i["G"], torch.float64)
    want = _grid_sample_gradients(i)
    for g, wnt, what in zip(got, want, ("ref", "src", "vis")):
        assert g.shape == wnt.shape and g.dtype == torch.float64
        assert wnt.abs().max() > 0.1
        assert (g - wnt).abs().max() <= 1e-12 * wnt.abs().max(), what


def test_float32_reference_is_fp32_class():
    """The unit of the GPU tests' bar: the same formulation in float32 is 1e-7 .. 3e-7 of the gradient's scale from float64."""
    (r64, r32) = R.case_reference("legacy-2x8x40x24x130")
    for a, b in zip(r32, r64):
        assert a.dtype == torch.float32
        assert 2.0 ** -25 < (a.double() - b).abs().max() / b.abs().max() < 2.0 ** -20


def test_constants_are_read_from_the_source(tmp_path):
    k = R.kernel_constants()
    assert k["TILE_X"] * k["TILE_Y"] == 256 and k["BOX"] > 0 and k["MAX_VIEWS"] == 8
    with pytest.raises((AssertionError, FileNotFoundError)):
        R.kernel_constants(str(tmp_path))


def test_segments_follow_the_launcher():
    k = R.kernel_constants()
    assert (k["TILE_X"], k["TILE_Y"], k["MIN_WGS"], k["MIN_PLANES"]) == (64, 4, 1024, 8), "the cases below are hand-computed for these"
    assert R.segments(2, 8, 17, 10, 70) == (2, 9)            # 9 + 8
    assert R.segments(2, 8, 33, 9, 66) == (4, 9)             # 9 + 9 + 9 + 6
    assert R.segments(1, 8, 15, 8, 20) == (1, 15)
    assert R.segments(3, 8, 40, 40, 130) == (4, 10) == R.segments(3, 32, 40, 40, 130)
    assert R.segments(6, 32, 48, 264, 480) == (1, 48)        # a training-size stage: already over 1024 workgroups


def test_box_plan_on_an_identity_warp():
    """Source camera = reference camera: every sample sits on its own pixel, so the box of a tile is the tile plus one texel to the
    right and below (clipped to the image), for every segment; nothing is empty."""
    from cds_mvsnet_amd import synth
    h, w, D = 8, 70, 16
    cams = synth.stage_cameras(2, h, w, seed=3)
    cams[0, 1] = cams[0, 0]
    hyp = synth.make_hypotheses(D, h, w, seed=4)
    boxes = R.box_plan(cams, hyp, 1, 8)
    nseg = R.segments(1, 8, D, h, w)[0]
    want = []
    for ty in (0, 4):
        for tx, tw in ((0, 64), (64, 6)):
            want += [(min(tx + tw, w - 1) - tx + 1) * (min(ty + 4, h - 1) - ty + 1)] * nseg
    # positions are computed in fp32: a sample may land a hair left of / above its pixel, which widens a box by one row or column
    assert len(boxes) == len(want)
    for b, wnt, (bw, bh) in zip(boxes, want, [(65, 5)] * nseg + [(6, 5)] * nseg + [(65, 4)] * nseg + [(6, 4)] * nseg):
        assert wnt <= b <= (bw + 1) * (bh + 1), (b, wnt)


def test_input_w_mixes_boxed_fallback_and_empty_workgroups():
    """The preconditions of the W cases of the GPU suite, per channel group: of the non-empty workgroups at least 25 % are clearly over
    the box budget (direct global atomics) and at least 25 % clearly under it (LDS box); at least 10 % of all are empty."""
    k = R.kernel_constants()
    boxes = R.case_box_plan("W-8")
    assert boxes == R.case_box_plan("W-32")                                     # the plan is per channel group
    assert len(boxes) == 30 * 3 * R.segments(3, 8, 40, 40, 130)[0]               # tiles x views x depth segments
    live = [b for b in boxes if b > 0]
    assert sum(b > 1.12 * k["BOX"] for b in live) >= 0.25 * len(live)
    assert sum(b < 0.88 * k["BOX"] for b in live) >= 0.25 * len(live)
    assert len(boxes) - len(live) >= 0.10 * len(boxes)
    assert max(boxes) == 40 * 130                                               # some workgroup's samples span the whole source image


def test_friendly_cases_never_leave_the_box():
    """What the five shapes of test_warp_aggregate_backward_vs_autograd (and the other friendly-geometry cases) do NOT cover: no
    workgroup comes near the box budget, so the fallback to global atomics never runs on them."""
    k = R.kernel_constants()
    for name in R.CASES:
        if not name.startswith("W-"):
            boxes = R.case_box_plan(name)
            assert 0 < max(boxes) <= 0.5 * k["BOX"], (name, max(boxes))
    assert len(R.LEGACY_SHAPES) == 5 and sum(n.startswith("legacy-") for n in R.CASES) == 5


def test_case_shapes():
    for name, (V, C, D, h, w) in R.CASES.items():
        i = R.case_input(name)
        assert i["ref"].shape == i["src"].shape == (V, C, h, w) and i["vis"].shape == (V, h, w) and i["G"].shape == (C, D, h, w)
        assert i["cams"].shape == (1, V + 1, 2, 4, 4) and i["hyp"].shape in ((1, D, h, w), (1, D))
    assert R.case_input("shared-hyp")["hyp"].dim() == 2 and R.CASES["nine-views"][0] > R.kernel_constants()["MAX_VIEWS"]
