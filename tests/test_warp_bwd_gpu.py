"""The warp-aggregate (K3) backward kernels of csrc/warp_bwd.hip against a float64 reference (tests/warp_bwd_ref.py), path by path:
the default kernel (scatter privatised in an LDS box, per-workgroup fallback to global atomics when the box is over budget, the
M == 0 and non-finite-M branches) and the run-merging direct kernel behind CDS_K3BWD_DIRECT=1, per-pixel and shared hypotheses,
one to four depth segments, more than MAX_VIEWS views, and the autograd wrapper ops.WarpAggregate.

Bar of each of the three gradients: train3d_ref.fp32_class_bar(r64, r32, margin=4.0) = 4 x the error of the same pass in float32 on
the CPU + one ulp of the gradient's scale.  Every test prints err / err32 before it asserts (profiles/k3_bwd_parity.md records them).
The preconditions - which workgroups of a case are boxed, fall back or are empty - are proven in tests/test_warp_bwd_ref_cpu.py.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_bwd_ref as R  # noqa: E402
from train3d_ref import fp32_class_bar  # noqa: E402

pytestmark = pytest.mark.gpu

KERNELS = ["default", "direct"]
WHAT = ("ref", "src", "vis")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from cds_mvsnet_amd import ops as o
    return o


def _select(monkeypatch, kernel):
    if kernel == "direct":
        monkeypatch.setenv("CDS_K3BWD_DIRECT", "1")        # the launcher reads it on every call
    else:
        monkeypatch.delenv("CDS_K3BWD_DIRECT", raising=False)


def _device_args(i, dev, vis=None, G=None):
    from cds_mvsnet_amd import geometry
    vis = i["vis"] if vis is None else vis
    G = i["G"] if G is None else G
    return (i["ref"].to(dev).contiguous(), i["src"].permute(0, 2, 3, 1).contiguous().to(dev), vis.to(dev).contiguous(),
            geometry.warp_matrices(i["cams"][0]), i["hyp"][0].to(dev).contiguous(), G.to(dev).contiguous())


def _backward(ops, dev, i, vis=None, G=None):
    """(g_ref [V,C,h,w], g_src [V,C,h,w], g_vis [V,h,w]) of ops.warp_aggregate_bwd on the CPU (g_src comes back channels-last)."""
    g_ref, g_src, g_vis = ops.warp_aggregate_bwd(*_device_args(i, dev, vis, G))
    return g_ref.cpu(), g_src.permute(0, 3, 1, 2).contiguous().cpu(), g_vis.cpu()


def _check(label, got, r64, r32, keep=None):
    """Every gradient within its bar; keep: optional boolean masks (one per gradient) of the entries compared (the scale and the fp32
    error are taken over all entries of the reference, which is finite everywhere)."""
    bad = []
    for k, what in enumerate(WHAT):
        err32, bar = fp32_class_bar(r64[k], r32[k], margin=4.0)
        diff = (got[k].double() - r64[k]).abs()
        if keep is not None:
            diff = diff[keep[k]]
        err = diff.max().item()
        print("K3BWD %s g_%s: err %.3e err32 %.3e err/err32 %.2f bar/err32 %.2f scale %.3e" %
              (label, what, err, err32, err / max(err32, 1e-300), bar / max(err32, 1e-300), r64[k].abs().max().item()))
        if not err <= bar:
            bad.append((what, err, bar))
    assert not bad, (label, bad)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_warp_aggregate_bwd_vs_float64(name, kernel, dev, ops, monkeypatch):
    """Friendly geometry (every workgroup boxed or empty) with 1, 2 and 4 depth segments, a short last segment, a tile remainder,
    shared hypotheses and nine views (two launches); input W at C = 8, 16, 32, where one launch of the default kernel mixes boxed
    workgroups, workgroups over the box budget (direct global atomics) and empty ones, and where the direct kernel's run merging meets
    a new texel cell on almost every plane."""
    _select(monkeypatch, kernel)
    r64, r32 = R.case_reference(name)
    got = _backward(ops, dev, R.case_input(name))
    _check("%s %s" % (name, kernel), got, r64, r32)


def test_autograd_wrapper_on_w(dev, ops, monkeypatch):
    """ops.WarpAggregate.apply + backward on W at C = 8 with a NON-contiguous channels-last source (a permuted view of a planar leaf),
    non-contiguous visibilities and a non-contiguous upstream gradient: the wrapper's .contiguous() calls, its layout and ctx.mats are
    held to the same bar."""
    from cds_mvsnet_amd import geometry
    _select(monkeypatch, "default")
    i = R.case_input("W-8")
    r64, r32 = R.case_reference("W-8")
    V, C, h, w = i["ref"].shape
    ref = i["ref"].to(dev).requires_grad_(True)
    src = i["src"].to(dev).requires_grad_(True)                                    # planar leaf: its gradient arrives through the permute
    vis2 = torch.stack((i["vis"], i["vis"]), dim=-1).to(dev).requires_grad_(True)  # [V, h, w, 2]: vis2[..., 0] is strided
    G2 = torch.stack((i["G"], -i["G"]), dim=-1).to(dev)
    vol = ops.WarpAggregate.apply(ref, src.permute(0, 2, 3, 1), vis2[..., 0], geometry.warp_matrices(i["cams"][0]), i["hyp"][0].to(dev))
    assert not src.permute(0, 2, 3, 1).is_contiguous() and not vis2[..., 0].is_contiguous() and not G2[..., 0].is_contiguous()
    vol.backward(G2[..., 0])
    assert vis2.grad[..., 1].abs().max().item() == 0.0
    _check("W-8 autograd", (ref.grad.cpu(), src.grad.cpu(), vis2.grad[..., 0].cpu()), r64, r32)


# ------------------------------------------------------------------------------------------------
# zero branches and a non-finite gradient (default kernel)
# ------------------------------------------------------------------------------------------------
def _zero_input():
    return R.case_input("legacy-%dx%dx%dx%dx%d" % R.ZERO_SHAPE)


def _reference_of(i, vis, G):
    V, _, h, w = i["ref"].shape
    pos = R.positions(i["cams"], i["hyp"], V, h, w)
    return tuple(R.reference((i["ref"], i["src"]), i["cams"], i["hyp"], vis, G, dt, pos) for dt in (torch.float64, torch.float32))


def test_zero_upstream_gradient_gives_exact_zeros(dev, ops, monkeypatch):
    """G == 0: M == 0 in every workgroup (no scatter at all), and all three gradients are exactly zero."""
    _select(monkeypatch, "default")
    i = _zero_input()
    for g in _backward(ops, dev, i, G=torch.zeros_like(i["G"])):
        assert torch.count_nonzero(g) == 0 and torch.isfinite(g).all()


def test_zero_visibility_still_gives_grad_vis(dev, ops, monkeypatch):
    """vis == 0: every contribution to grad_src is zero (M == 0: the scatter is skipped) and grad_ref = vis * (...) is zero, but
    grad_vis = sum_{c,d} g ref warp is not: the branch that skips the scatter must still produce it."""
    _select(monkeypatch, "default")
    i = _zero_input()
    vis = torch.zeros_like(i["vis"])
    r64, r32 = _reference_of(i, vis, i["G"])
    assert r64[0].abs().max() == 0 and r64[1].abs().max() == 0 and r64[2].abs().max() > 1.0
    g_ref, g_src, g_vis = _backward(ops, dev, i, vis=vis)
    assert torch.count_nonzero(g_ref) == 0 and torch.count_nonzero(g_src) == 0
    assert g_vis.abs().max() > 0
    _check("vis=0 default", (g_ref, g_src, g_vis), r64, r32)


def test_partly_zero_gradient_and_visibility(dev, ops, monkeypatch):
    """G zeroed on rows 8..15 (two rows of tiles whose workgroups have M == 0 next to ordinary ones) and vis zeroed on rows 16..19
    (one row of tiles with M == 0 but a non-zero grad_vis): all three gradients within the bar."""
    _select(monkeypatch, "default")
    i = _zero_input()
    G, vis = i["G"].clone(), i["vis"].clone()
    G[:, :, 8:16] = 0
    vis[:, 16:20] = 0
    r64, r32 = _reference_of(i, vis, G)
    assert r64[2][:, 16:20].abs().max() > 1.0 and r64[2][:, 8:16].abs().max() == 0
    _check("partly zero default", _backward(ops, dev, i, vis=vis, G=G), r64, r32)


def _full_weight_voxel(i):
    """(c, d, y, x) whose view-0 sample has all four taps inside the source image, each with weight > 0.01 (the first in plane order
    from the middle of the volume on), and per view the taps (x, y) of that voxel's sample that are inside."""
    V, C, h, w = i["ref"].shape
    pos = R.positions(i["cams"], i["hyp"], V, h, w)
    t0 = R.taps(pos[0][0], pos[0][1], h, w)
    good = torch.stack([ok & (wt > 0.01) for _, _, wt, ok in t0]).all(0)                 # [D, hw]
    D = good.shape[0]
    idx = torch.nonzero(good[D // 2:].reshape(-1))[0].item() + (D // 2) * h * w
    d, p = divmod(idx, h * w)
    inside = []
    for v in range(V):
        inside.append([(int(xi[d, p]), int(yi[d, p])) for xi, yi, _, ok in R.taps(pos[v][0], pos[v][1], h, w) if bool(ok[d, p])])
    return (C // 2, d, p // w, p % w), inside


def test_non_finite_upstream_gradient_propagates_where_it_belongs(dev, ops, monkeypatch):
    """The documented contract "non-finite M takes the fp32 direct scatter, which propagates it": one inf in G makes grad_src non-finite
    at exactly the taps (inside the image) of that voxel's sample in the voxel's channel - for view 0 these are four texels -, and
    grad_ref[v, c, y, x] / grad_vis[v, y, x] for every view whose sample there has a tap inside.  Every other entry is finite and within
    the bar of the reference computed with that entry of G set to zero (its workgroup scatters with fp32 global atomics instead of
    the box: still fp32-class)."""
    _select(monkeypatch, "default")
    i = _zero_input()
    V, C, h, w = i["ref"].shape
    (c, d, y, x), inside = _full_weight_voxel(i)
    assert len(inside[0]) == 4
    G_inf, G_0 = i["G"].clone(), i["G"].clone()
    G_inf[c, d, y, x] = float("inf")
    G_0[c, d, y, x] = 0.0
    r64, r32 = _reference_of(i, i["vis"], G_0)
    want = [torch.zeros(V, C, h, w, dtype=torch.bool), torch.zeros(V, C, h, w, dtype=torch.bool), torch.zeros(V, h, w, dtype=torch.bool)]
    for v in range(V):
        for tx, ty in inside[v]:
            want[1][v, c, ty, tx] = True
        if inside[v]:
            want[0][v, c, y, x] = True
            want[2][v, y, x] = True
    assert int(want[1][0].sum()) == 4
    got = _backward(ops, dev, i, G=G_inf)
    for g, wnt, what in zip(got, want, WHAT):
        nonfinite = ~torch.isfinite(g)
        assert torch.equal(nonfinite, wnt), ("g_" + what, "non-finite at", torch.nonzero(nonfinite).tolist(), "expected", torch.nonzero(wnt).tolist())
    _check("one inf default", got, r64, r32, keep=[~m for m in want])
