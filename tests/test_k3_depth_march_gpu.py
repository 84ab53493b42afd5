"""GPU tests of the DEPTH MARCH of K3 (warp_aggregate_lds_kernel) and K1 (warp_entropy_lds_kernel), csrc/warp_lds.hip: a workgroup
that walks several LDS chunks, chunks that are halved (48 -> 24 -> 12 -> 6) and still staged, chunk starts off the 48-plane grid, a
one-plane last chunk, the global-memory fallback between staged chunks, and the accumulating second launch of 5 - 7 views reading its
partial sums one plane pair ahead across chunk boundaries.  The small oracle cases of test_hip_parity.py never run that march: their
launcher gives every workgroup exactly one chunk, and their geometry never halves one.  Here CDS_K3_NSEG forces 1 or 2 depth segments
and two input families make the march long (A) or halving (B); tests/k3_chunk_plan.py (a CPU model, used only for PRECONDITIONS on the
inputs) proves that each B case really contains the halved chunks it is meant to test.

Reference: the CPU oracle exactly as test_warp_kernels_vs_oracle_odd_shapes builds it (O.warp_volume, O.correlation_entropy,
visibility-weighted sum in view order, / (vis_sum + 1e-6)), cached per (input, D, C, view) because it does not depend on the layout,
the segments or the position mode.  Tolerances are the project's own: volume 1e-5 (exact positions) / 5e-5 (fast), entropy 5e-5 / 2e-4,
vis_sum 1e-6, unnormalised sums 2e-5.  Every non-accumulating K3 call gets a volume pre-filled with NaN and must return a finite one:
a voxel that no chunk wrote is a failure.

Oracle cost (16 host threads, measured in one run): the per-view oracle results of all small cases together take 15.4 s (printed
when the module's tests are done), against 18.9 s for the single O.stage_forward of the existing `M1 full size` case in the same run
(20.9 s in another).  That limit shaped the case list: a first list with C = 32 on six views of input B took 49 s.  The two config-4
cases take 6.6 + 6.8 s more (see test_oracle_parity_config4_stage1).
"""
import collections
import os
import subprocess
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k3_chunk_plan as plan  # noqa: E402

pytestmark = pytest.mark.gpu

POISON_PATTERNS = ("7fc00000", "00000000")      # a quiet NaN / zeros in every LDS word before each launch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    yield torch.device("cuda:0")
    print("\noracle time of the depth-march cases (per-view results, cached): %.1f s" % ORACLE_SECONDS[0])


@pytest.fixture(scope="module")
def ops():
    from cds_mvsnet_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------
# inputs and the oracle
# ------------------------------------------------------------------------------------------------
_FEATS = {}
_ORACLE = collections.OrderedDict()
_ORACLE_BUDGET = 1200 * 1000 * 1000    # floats kept (4.8 GB; all cases together need 0.7 G: nothing is computed twice): B at C = 32 is 47.5 M per view
ORACLE_SECONDS = [0.0]


def _features(name, C):
    from cds_mvsnet_amd import synth
    if (name, C) not in _FEATS and name == "W":
        _FEATS[(name, C)] = plan.w_features(C)
    if (name, C) not in _FEATS:
        cams, hyp = plan.named_input(name, plan.B_DEPTH if name.startswith("B") else 96)
        _, _, h, w = hyp.shape
        _FEATS[(name, C)] = synth.make_pair_features(plan.N_SRC, C, h, w, seed=70 + C + len(name), sharp=True)
    return _FEATS[(name, C)]


def _oracle_view(name, D, C, view):
    """(in_prod [C, D, h, w], entropy [h, w], share of non-zero warped samples) of camera `view` (>= 1), fp32 CPU oracle."""
    from oracle import cds_oracle as O
    key = (name, D, C, view)
    if key in _ORACLE:
        _ORACLE.move_to_end(key)
        return _ORACLE[key]
    t0 = time.time()
    cams, hyp = plan.named_input(name, D)
    f = _features(name, C)[view - 1]
    warped = O.warp_volume(f["src"][0], O.compose_projection(cams[:, view]), O.compose_projection(cams[:, 0]), hyp)
    in_prod, e = O.correlation_entropy(f["ref"][0], warped)
    _ORACLE[key] = (in_prod[0], e[0, 0], float((warped != 0).float().mean()))
    while sum(v[0].numel() for v in _ORACLE.values()) > _ORACLE_BUDGET and len(_ORACLE) > 1:
        _ORACLE.popitem(last=False)
    ORACLE_SECONDS[0] += time.time() - t0
    return _ORACLE[key]


def _vis(name, D):
    _, hyp = plan.named_input(name, D)
    _, _, h, w = hyp.shape
    return torch.rand(plan.N_SRC, h, w, generator=torch.Generator().manual_seed(1)) * 0.8 + 0.1


def _oracle_volume(name, D, C, views, normalize=True):
    vis = _vis(name, D)
    vol = 0.0
    for v in views:
        vol = vol + _oracle_view(name, D, C, v)[0] * vis[v - 1]
    vis_sum = vis[[v - 1 for v in views]].sum(0)
    return (vol / (vis_sum + 1e-6) if normalize else vol), vis_sum


def _device_inputs(name, D, C, views, dev, ops):
    from cds_mvsnet_amd import geometry
    cams, hyp = plan.named_input(name, D)
    f = _features(name, C)
    ref = torch.stack([f[v - 1]["ref"][0][0] for v in views]).to(dev).contiguous()
    src = torch.stack([ops.chw_to_hwc(f[v - 1]["src"][0][0].to(dev).contiguous()) for v in views])
    mats = geometry.warp_matrices(cams[0])[[v - 1 for v in views]].contiguous()
    vis = _vis(name, D)[[v - 1 for v in views]].to(dev).contiguous()
    return ref, src, vis, mats, hyp[0].to(dev).contiguous()


def _k3(ops, dev, ref, src, vis, mats, hyp_d, channels_last=False, exact=True, normalize=True, window=None):
    """K3 into a NaN-filled volume; returns (volume as [C, D, h, w] on the CPU, vis_sum on the CPU).  Finite everywhere or it fails."""
    V, C, h, w = ref.shape
    D = hyp_d.shape[0]
    out = torch.full((D, h, w, C) if channels_last else (C, D, h, w), float("nan"), device=dev)
    vol, vis_sum = ops.warp_aggregate(ref, src, vis, mats, hyp_d, normalize=normalize, volume=out, channels_last=channels_last,
                                      exact=exact, window=window)
    assert vol.data_ptr() == out.data_ptr()
    vol = vol.permute(3, 0, 1, 2) if channels_last else vol
    assert torch.isfinite(vol).all(), "K3 left %d voxels unwritten / non-finite" % int((~torch.isfinite(vol)).sum())
    return vol.cpu(), vis_sum.cpu()


def _set_env(monkeypatch, nseg=None, split=None):
    for key, val in (("CDS_K3_NSEG", nseg), ("CDS_K3_SPLIT", split)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(val))


def _check_nonzero(name, D, C, views):
    for v in views:
        share = _oracle_view(name, D, C, v)[2]
        assert share >= 0.60, "view %d of %s: only %.0f %% of the warped samples are non-zero" % (v, name, 100 * share)


def _is_b(name):
    return name.startswith("B")


# ------------------------------------------------------------------------------------------------
# 1. multi-chunk march against the oracle
# ------------------------------------------------------------------------------------------------
# (input, D, source views (camera indices), C, CDS_K3_NSEG (None = unset), channels_last, exact, normalize)
# every V in 1..4 and every C at least twice; B launches are chosen so that their preconditions hold (view 1 or 5 alone halves too
# rarely: the one-view B case uses view 2).  The oracle of input B costs 47.5 M voxels per view at C = 32: to keep the oracle time of all
# small cases below that of the M1 full-size case, B runs C = 32 on view 2 only, C = 16 on views 1 - 2 and C = 8 on all seven;
# C = 32 with four views and C = 16 / 32 in the accumulating launch are covered on families A / A2.
MARCH_CASES = [
    ("A", 96, (1,), 8, 1, False, True, True),
    ("A", 97, (1, 2), 16, 1, True, True, True),
    ("A", 97, (1, 2, 3, 4), 8, None, False, False, True),
    ("A", 120, (1, 2, 3), 8, 1, False, True, False),
    ("A2", 120, (1, 2, 3), 32, 1, False, True, False),
    ("A", 145, (1, 2, 3, 4), 8, 1, True, True, True),
    ("A", 145, (1, 2), 32, 2, False, False, True),
    ("A", 145, (1, 2, 3), 8, 2, True, True, False),
    ("A", 192, (1,), 16, 1, True, False, True),
    ("A", 192, (1, 2, 3, 4), 8, 2, False, True, True),
    ("A", 194, (1, 2, 3), 8, 1, False, True, True),
    ("A", 194, (1, 2), 8, 2, True, True, False),
    ("A2", 97, (1, 2, 3), 8, 1, True, False, True),
    ("A2", 145, (1, 2, 3, 4), 16, 1, False, True, True),
    ("A2", 194, (1,), 32, None, False, True, True),
    ("A2", 120, (1, 2), 8, 2, False, True, True),
    ("B", 145, (2,), 8, 1, False, True, True),
    ("B", 145, (1, 2), 16, 1, True, True, True),
    ("B", 145, (1, 2, 3), 8, 1, False, True, True),
    ("B", 145, (1, 2, 3), 8, 2, True, False, True),
    ("B", 145, (2,), 32, 2, False, True, True),
    ("B", 145, (1, 2, 3, 4), 8, 1, True, True, True),
    ("B", 145, (1, 2, 3, 4), 8, None, False, True, True),
    ("B", 145, (1, 2), 16, 1, True, False, True),
    ("B", 145, (4, 5, 6), 8, 1, True, True, False),
    ("B", 145, (2,), 16, None, True, True, False),
    ("Bperm", 145, (1, 2, 3), 8, 1, False, True, True),
    ("Bperm", 145, (1, 2, 3, 4), 8, 2, True, True, True),
    ("Bperm", 145, (4, 5, 6), 8, 1, True, False, False),
    ("Bperm", 145, (4, 5, 6), 8, 1, True, True, False),
]


def _case_id(c):
    return "-".join("v" + "".join(map(str, x)) if isinstance(x, tuple) else str(x) for x in c)


@pytest.mark.parametrize("name,D,views,C,nseg,cl,exact,normalize", MARCH_CASES, ids=[_case_id(c) for c in MARCH_CASES])
def test_k3_multi_chunk_march_vs_oracle(name, D, views, C, nseg, cl, exact, normalize, dev, ops, monkeypatch):
    """One workgroup marching over several chunks (CDS_K3_NSEG = 1: all of them; 2: half; unset: the launcher's choice), every view
    count's specialisation, C = 8 / 16 / 32, both layouts, both position modes, normalised or raw sums, against the CPU oracle."""
    if _is_b(name):
        plan.assert_halving_input(name, D, views)
    _set_env(monkeypatch, nseg)
    want, want_vs = _oracle_volume(name, D, C, views, normalize)
    if _is_b(name):
        _check_nonzero(name, D, C, views)
    ref, src, vis, mats, hyp_d = _device_inputs(name, D, C, views, dev, ops)
    vol, vis_sum = _k3(ops, dev, ref, src, vis, mats, hyp_d, channels_last=cl, exact=exact, normalize=normalize)
    err = (vol - want).abs().max().item()
    print("volume max-abs vs oracle", err)
    if normalize or exact:
        assert err < ((1e-5 if exact else 5e-5) if normalize else 2e-5)
    else:
        # Raw sums with FAST positions: 2e-5 is the bound of the arithmetic, not of the fast mode's position error (~1e-7 w px), which the
        # normalised cases allow 5e-5 for.  A raw sum is the normalised value times (vis_sum + 1e-6), so the same 5e-5 is asked of
        # error / (vis_sum + 1e-6).  Measured on the CPU for Bperm, views 4 - 6, C = 8: shifting the fp32 oracle's sample positions by
        # +-1e-7 w px moves its raw sums by up to 1.0e-4 and their normalised form by 4.6e-5; the kernel's raw sums differ from the
        # oracle by 4.5e-5 there, inside what the position error alone explains (exact mode on the same kind of input: < 2e-5).
        err_n = ((vol - want).abs() / (want_vs + 1e-6)).max().item()
        print("raw sums, fast positions: max-abs error / (vis_sum + 1e-6)", err_n)
        assert err_n < 5e-5
    assert (vis_sum - want_vs).abs().max() < 1e-6


# (input, D, views, C, exact).  K1 has no segment knob: every workgroup marches all chunks of its (tile, view).  C = 8 is the 64-plane /
# 1016-texel instantiation (97 = 64 + 33, 145 = 64 + 64 + 17: odd last pairs), C = 16 / 32 the 48-plane / 632-texel one.  K1's own halving
# precondition at C = 8 (>= 10 % of the chunks halved and staged, its box being larger) already holds on input B with lo = 150 (the model
# gives 18 - 20 % over views 1 - 4), so B' = B: no lower `lo` was needed.
K1_CASES = [
    ("A", 96, (1, 2), 8, True), ("A", 97, (1, 2, 3), 8, True), ("A", 97, (1,), 16, False), ("A", 120, (1, 2), 32, True),
    ("A", 145, (1, 2, 3, 4), 8, False), ("A", 145, (1, 2), 16, True), ("A", 192, (1, 2, 3), 8, True), ("A", 194, (1, 2), 8, True),
    ("A", 194, (1,), 16, True), ("A2", 145, (1, 2, 3), 8, True), ("A2", 97, (1, 2), 32, False),
    ("B", 145, (1, 2, 3, 4), 8, True), ("B", 145, (2, 3, 4), 8, False), ("B", 145, (1, 2), 16, True), ("B", 145, (2,), 32, True),
    ("Bperm", 145, (1, 2, 3, 4), 8, True), ("Bperm", 145, (2, 3, 4), 8, False),
]


@pytest.mark.parametrize("name,D,views,C,exact", K1_CASES, ids=[_case_id(c) for c in K1_CASES])
def test_k1_multi_chunk_march_vs_oracle(name, D, views, C, exact, dev, ops):
    if _is_b(name):
        plan.assert_k1_halving_input(name, D, views, C)
    want = torch.stack([_oracle_view(name, D, C, v)[1] for v in views])
    assert torch.isfinite(want).all()
    if _is_b(name):
        _check_nonzero(name, D, C, views)
    ref, src, vis, mats, hyp_d = _device_inputs(name, D, C, views, dev, ops)
    ent = ops.warp_entropy(ref, src, mats, hyp_d, exact=exact).cpu()
    err = (ent - want).abs().max().item()
    print("entropy max-abs vs oracle", err)
    assert err < (5e-5 if exact else 2e-4)


# ------------------------------------------------------------------------------------------------
# 1b. wild geometry that hits the image: (nearly) every chunk on the global-memory path
# ------------------------------------------------------------------------------------------------
W_VIEWS = (1, 2, 3)
W_D = plan.W_SHAPE[1]


def w_oracle_content(C):
    """Share of the entries of the oracle's un-normalised volume of input W (all three views) that are finite and above 1e-3 in
    magnitude: the wild-geometry test compares content, not zeros."""
    want, _ = _oracle_volume("W", W_D, C, W_VIEWS, normalize=False)
    return float((torch.isfinite(want) & (want.abs() > 1e-3)).float().mean())


def _max_err(got, want):
    ok = torch.isfinite(want)
    return (got - want).abs()[ok].max().item(), float(ok.float().mean())


@pytest.mark.parametrize("C", [8, 16])
def test_k3_k1_wild_geometry_w_vs_oracle(C, dev, ops):
    """Input W: hypotheses drawn independently per pixel and plane, a wide baseline and a view whose z = 0 plane cuts the sweep, with the
    samples still INSIDE the source images (test_warp_lds_fallbacks_wild_geometry of test_hip_parity.py has the same kind of geometry but
    not one sample inside: it compares zeros).  Every chunk of K3 over three views, 94 % over two, 75 % / 92 % of K1's (C = 8 / 16) take the
    global-memory path, so this is the test of the values that path produces.  Exact positions, all three views: un-normalised volume
    2e-5 on the oracle's finite entries (at least 99 % of all), entropy 5e-5 where the oracle's is finite - the bounds of the older wild
    test.  Fast positions, views 1 - 2 (the pole view's samples are a question of position sensitivity, not of the kernel): normalised
    volume 5e-5, entropy 2e-4, the bounds of test_warp_kernels_vs_oracle_odd_shapes for fast positions at widths up to 130."""
    frac = plan.assert_wild_input()
    content = w_oracle_content(C)
    print("in-image fractions", frac, "oracle entries finite and > 1e-3: %.3f" % content)
    assert content >= 0.5
    ref, src, vis, mats, hyp_d = _device_inputs("W", W_D, C, W_VIEWS, dev, ops)
    # exact positions, all three views
    want, _ = _oracle_volume("W", W_D, C, W_VIEWS, normalize=False)
    out = torch.full((C, W_D) + tuple(ref.shape[2:]), float("nan"), device=dev)
    vol, _ = ops.warp_aggregate(ref, src, vis, mats, hyp_d, normalize=False, volume=out, exact=True)
    err, finite = _max_err(vol.cpu(), want)
    print("exact: un-normalised volume max-abs vs oracle %.3g (oracle finite on %.4f)" % (err, finite))
    assert finite >= 0.99
    assert err < 2e-5
    ent = ops.warp_entropy(ref, src, mats, hyp_d, exact=True).cpu()
    for i, v in enumerate(W_VIEWS):
        err, finite = _max_err(ent[i], _oracle_view("W", W_D, C, v)[1])
        print("exact: entropy of view %d max-abs vs oracle %.3g (oracle finite on %.4f)" % (v, err, finite))
        assert err < 5e-5
    # fast positions, views 1 - 2, normalised
    want, _ = _oracle_volume("W", W_D, C, W_VIEWS[:2], normalize=True)
    out = torch.full((C, W_D) + tuple(ref.shape[2:]), float("nan"), device=dev)
    vol, _ = ops.warp_aggregate(ref[:2], src[:2], vis[:2], mats[:2], hyp_d, normalize=True, volume=out, exact=False)
    err, finite = _max_err(vol.cpu(), want)
    print("fast: normalised volume of views 1 - 2 max-abs vs oracle %.3g (oracle finite on %.4f)" % (err, finite))
    assert finite >= 0.99
    assert err < 5e-5
    ent = ops.warp_entropy(ref[:2], src[:2], mats[:2], hyp_d, exact=False).cpu()
    for i, v in enumerate(W_VIEWS[:2]):
        err, _ = _max_err(ent[i], _oracle_view("W", W_D, C, v)[1])
        print("fast: entropy of view %d max-abs vs oracle %.3g" % (v, err))
        assert err < 2e-4


# ------------------------------------------------------------------------------------------------
# 2. the accumulating second launch across chunk boundaries
# ------------------------------------------------------------------------------------------------
# (input, D, views, C, CDS_K3_NSEG, channels_last, CDS_K3_SPLIT (None: the default (V + 1) / 2)).  Default splits: 5 = 3 + 2, 6 = 3 + 3,
# 7 = 4 + 3; CDS_K3_SPLIT 4 / 2 / 3 give 4 + 1, 2 + 4, 3 + 4, so the accumulating launch runs in its 1-, 2-, 3- and 4-view specialisations.
# On B the accumulating launch's views are chosen so that IT meets the halving preconditions (view 5 alone does not: the 4 + 1 case on
# B ends with view 2).
ACC_CASES = [
    ("A", 97, (1, 2, 3, 4, 5), 8, 1, False, None),
    ("A", 97, (1, 2, 3, 4, 5, 6), 16, 2, True, None),
    ("A", 97, (1, 2, 3, 4, 5, 6), 8, 2, True, 2),
    ("A", 145, (1, 2, 3, 4, 5, 6, 7), 8, 1, True, None),
    ("A2", 97, (1, 2, 3, 4, 5), 32, 2, False, None),
    ("A", 145, (1, 2, 3, 4, 5), 8, 1, False, 4),
    ("A", 145, (1, 2, 3, 4, 5, 6, 7), 8, 2, False, 3),
    ("A2", 145, (1, 2, 3, 4, 5, 6), 8, 1, False, None),
    ("B", 145, (1, 2, 3, 4, 5), 8, 1, False, None),
    ("B", 145, (1, 2, 3, 4, 5, 6), 8, 1, True, None),
    ("B", 145, (1, 2, 3, 4, 5, 6), 8, 2, True, None),
    ("B", 145, (1, 2, 3, 4, 5, 6, 7), 8, 2, False, None),
    ("B", 145, (1, 3, 4, 5, 2), 8, 1, True, 4),
    ("B", 145, (1, 2, 3, 4, 5, 6), 8, 1, False, 2),
    ("B", 145, (1, 2, 3, 4, 5, 6, 7), 8, 1, True, 3),
    ("Bperm", 145, (1, 2, 3, 4, 5, 6), 8, 1, True, None),
]


@pytest.mark.parametrize("name,D,views,C,nseg,cl,split", ACC_CASES, ids=[_case_id(c) for c in ACC_CASES])
def test_k3_accumulating_launch_across_chunks_vs_oracle(name, D, views, C, nseg, cl, split, dev, ops, monkeypatch):
    """5 - 7 views = two launches; the second (ACCUMULATE) loads the first one's partial sums at each chunk's first plane pair, then
    one pair ahead, clamped to the chunk's last plane.  Here that launch crosses chunk boundaries (also halved and off-grid ones)."""
    launches = plan.k3_launch_views(views, split)
    assert len(launches) == 2
    if _is_b(name):
        plan.assert_halving_input(name, D, launches[1])
    _set_env(monkeypatch, nseg, split)
    want, want_vs = _oracle_volume(name, D, C, views)
    if _is_b(name):
        _check_nonzero(name, D, C, views)
    ref, src, vis, mats, hyp_d = _device_inputs(name, D, C, views, dev, ops)
    vol, vis_sum = _k3(ops, dev, ref, src, vis, mats, hyp_d, channels_last=cl)
    err = (vol - want).abs().max().item()
    print("volume max-abs vs oracle", err)
    assert err < 1e-5
    assert (vis_sum - want_vs).abs().max() < 1e-6


@pytest.mark.parametrize("name,D,C,cl,nseg", [("A", 145, 16, False, 1), ("B", 145, 8, True, 1), ("B", 145, 8, False, 2)])
def test_k3_caller_side_accumulate_two_plus_two_views(name, D, C, cl, nseg, dev, ops, monkeypatch):
    """The form the view-sharded path uses: accumulate=True onto an existing UNNORMALISED volume.  Two calls of 2 + 2 views against one
    call of 4 (one rounding per view: 2e-6, the bound of test_warp_paths_agree_lds_vs_direct) and against the oracle (2e-5)."""
    views = (1, 2, 3, 4)
    if _is_b(name):
        plan.assert_halving_input(name, D, views[2:])
    _set_env(monkeypatch, nseg)
    want, want_vs = _oracle_volume(name, D, C, views, normalize=False)
    ref, src, vis, mats, hyp_d = _device_inputs(name, D, C, views, dev, ops)
    one, vs_one = _k3(ops, dev, ref, src, vis, mats, hyp_d, channels_last=cl, normalize=False)
    out = torch.full((D,) + tuple(ref.shape[2:]) + (C,) if cl else (C, D) + tuple(ref.shape[2:]), float("nan"), device=dev)
    vs = torch.empty(ref.shape[2:], device=dev)
    ops.warp_aggregate(ref[:2], src[:2], vis[:2], mats[:2], hyp_d, normalize=False, volume=out, vis_sum=vs, channels_last=cl, exact=True)
    ops.warp_aggregate(ref[2:], src[2:], vis[2:], mats[2:], hyp_d, normalize=False, volume=out, vis_sum=vs, accumulate=True,
                       channels_last=cl, exact=True)
    two = (out.permute(3, 0, 1, 2) if cl else out).cpu()
    assert torch.isfinite(two).all()
    assert (two - one).abs().max() < 2e-6
    assert (two - want).abs().max() < 2e-5
    assert (vs.cpu() - want_vs).abs().max() < 1e-6 and (vs_one - want_vs).abs().max() < 1e-6


# ------------------------------------------------------------------------------------------------
# 3. segment invariance
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("name,D,V,C", [("A", 145, 4, 8), ("A", 145, 6, 16), ("B", 145, 4, 16), ("B", 145, 6, 8)])
def test_k3_volume_does_not_depend_on_depth_segments(name, D, V, C, cl, dev, ops, monkeypatch):
    """CDS_K3_NSEG = 1, 2, 3 and unset give the same volume BIT FOR BIT.  Another segmentation changes where chunks start, which of
    them are halved and so which plane pairs take the branch-free staged path, the per-lane redo (fetch_cell) or the global-memory
    path.  These are the same arithmetic: both paths call positions2 / plane_weights / interp8 with the same operands and add a view
    with ONE fma2(rv[v][j], o[j], acc) in view order from the same initial value (zero or the loaded partial sum times yden); a
    texel is the same number from LDS or from global memory, a zero-border texel times a weight equals a zeroed weight times a texel
    for finite features; the library is built with -ffp-contract=off, so neither copy of the code is contracted differently.  Hence
    torch.equal, not a tolerance."""
    views = tuple(range(1, V + 1))
    ref, src, vis, mats, hyp_d = _device_inputs(name, D, C, views, dev, ops)
    vols = {}
    for nseg in (1, 2, 3, None):
        _set_env(monkeypatch, nseg)
        vols[nseg], _ = _k3(ops, dev, ref, src, vis, mats, hyp_d, channels_last=cl)
    for nseg in (2, 3, None):
        assert torch.equal(vols[nseg], vols[1]), "CDS_K3_NSEG=%s differs from 1 by %g" % (nseg, (vols[nseg] - vols[1]).abs().max().item())


# ------------------------------------------------------------------------------------------------
# 4. row windows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,D,V,C,y0,y1", [("B", 145, 3, 8, 13, 43), ("B", 145, 6, 16, 5, 62), ("A", 145, 3, 16, 5, 19), ("A", 145, 6, 8, 3, 22)])
def test_k3_k1_row_windows_equal_full_grid_rows_on_long_marches(name, D, V, C, y0, y1, dev, ops, monkeypatch):
    """test_warp_row_windows_equal_full_grid_rows's assertion (the window's rows equal the full grid's rows bit for bit) where every
    workgroup marches several chunks (CDS_K3_NSEG = 1) and the windows start and end off the 8-row tile grid.  A window's tiles cover
    other pixel rows than the full grid's, so on input B they halve differently; the equality holds because the staged, redo and
    global-memory paths are the same arithmetic (see test_k3_volume_does_not_depend_on_depth_segments)."""
    views = tuple(range(1, V + 1))
    _set_env(monkeypatch, 1)
    ref, src, vis, mats, hyp_d = _device_inputs(name, D, C, views, dev, ops)
    h = ref.shape[2]
    ref_w, hyp_w, vis_w = ref[:, :, y0:y1].contiguous(), hyp_d[:, y0:y1].contiguous(), vis[:, y0:y1].contiguous()
    for exact in (True, False):
        ent_full = ops.warp_entropy(ref, src, mats, hyp_d, exact=exact)
        ent_w = ops.warp_entropy(ref_w, src, mats, hyp_w, exact=exact, window=(h, y0))
        assert torch.equal(ent_w, ent_full[:, y0:y1])
        for cl in (False, True):
            vol_full, vs_full = _k3(ops, dev, ref, src, vis, mats, hyp_d, channels_last=cl, exact=exact)
            vol_w, vs_w = _k3(ops, dev, ref_w, src, vis_w, mats, hyp_w, channels_last=cl, exact=exact, window=(h, y0))
            assert torch.equal(vs_w, vs_full[y0:y1])
            assert torch.equal(vol_w, vol_full[:, :, y0:y1])


# ------------------------------------------------------------------------------------------------
# 5. stale LDS between chunks
# ------------------------------------------------------------------------------------------------
STALE_CASES = {"A4": ("A", 145, 4, 8), "B4": ("B", 145, 4, 8), "A6": ("A", 145, 6, 16), "B6": ("B", 145, 6, 16)}


def _stale_lds_outputs(case, dev, ops):
    """K1 and K3 (planar and channels-last, one depth segment) of a case, as CPU tensors."""
    name, D, V, C = STALE_CASES[case]
    ref, src, vis, mats, hyp_d = _device_inputs(name, D, C, tuple(range(1, V + 1)), dev, ops)
    ent = ops.warp_entropy(ref, src, mats, hyp_d, exact=True).cpu()
    planar, vs = _k3(ops, dev, ref, src, vis, mats, hyp_d)
    cl, _ = _k3(ops, dev, ref, src, vis, mats, hyp_d, channels_last=True)
    return ent, planar, cl, vs


@pytest.mark.parametrize("case", ["A4", "B6", "B4", "A6"])
def test_results_do_not_depend_on_stale_lds(case, dev, ops, monkeypatch, tmp_path):
    """csrc/lib.hip's debug aid put to use: with CDS_DEBUG_POISON_LDS=<hex> every entry point synchronises and fills the LDS of every
    CU after its launch, so the next kernel starts on NaN (7fc00000) or zero LDS.  K1 / K3 marching several chunks - on B halved
    ones, whose boxes are smaller than the box of the longer chunk staged before them - must give bit-identical results under both
    patterns and without poisoning: the zero border of a box and the box of a halved chunk are really staged, nothing reads texels
    left over from an earlier chunk or workgroup.  The poisoned runs are child processes (the variable is read in the library), each
    under its own time limit; after a failed child nothing more is started."""
    monkeypatch.setenv("CDS_K3_NSEG", "1")
    outs = []
    for pattern in POISON_PATTERNS:
        path = str(tmp_path / ("poison_%s.pt" % pattern))
        env = dict(os.environ, CDS_DEBUG_POISON_LDS=pattern, CDS_K3_NSEG="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, path], env=env, timeout=300,
                           cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):     # killed by a signal: the GPU may be in a bad state
            pytest.exit("child with CDS_DEBUG_POISON_LDS=%s died with status %d: no further GPU test is started" % (pattern, r.returncode), 3)
        if r.returncode != 0:
            pytest.fail("child with CDS_DEBUG_POISON_LDS=%s ended with status %d: nothing more is run" % (pattern, r.returncode))
        outs.append(torch.load(path))
    monkeypatch.delenv("CDS_DEBUG_POISON_LDS", raising=False)
    outs.append(_stale_lds_outputs(case, dev, ops))
    for other in outs[:-1]:
        for a, b, what in zip(other, outs[-1], ("entropy", "planar volume", "channels-last volume", "vis_sum")):
            assert torch.equal(a, b), "%s depends on what the LDS held before the launch" % what


# ------------------------------------------------------------------------------------------------
# BASELINE config 4, stage 1, at its real shape
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg4", "cfg4near"])
def test_oracle_parity_config4_stage1(name, dev, ops, seeded_state):
    """Stage 1 of BASELINE config 4 (1920x1056, N = 7) at its real shape: 480x264, D = 48, C = 32, six source views through
    model.stage_net against O.stage_forward, asserted like test_oracle_parity_large_depth_range (volume 1e-5, depth mean-L1 1e-3,
    confidence 1e-3, norm_curv 1e-6).  Config 4 at full size was property-checked only.  `cfg4`: the default hypothesis range; the CPU
    model finds 45 % of its chunks halved (48 -> 24) already, in both launches.  `cfg4near`: lo = 300 instead of 425, the kind of range
    input B has: 61 % / 64 % of the chunks of the two launches halved, lengths 6 .. 42, none on the global-memory path.  CDS_K3_NSEG is
    left unset: the accumulating launch meets halved chunks at the tile and segment counts it really runs with.
    Oracle cost, measured in one run on the GPU machine's 16 host threads, each O.stage_forward in a process of its own: the existing
    `M1 full size` case 18.9 - 20.9 s and 11.3 GB peak resident memory; this case 6.6 s (cfg4) / 6.8 s (cfg4near) and 4.5 GB.  Both are well
    below the M1 case, so the whole 480-column grid is used, not a 240-column window."""
    from cds_mvsnet_amd import geometry, synth
    from oracle import cds_oracle as O
    h, w, D, C, N, stage = 264, 480, 48, 32, 7, 0
    k = plan.k3_constants()
    cams, hyp = plan.named_input(name, D)
    for views in plan.k3_launch_views(range(1, N)):
        p = plan.named_plan(name, D, views, k["dc"], k["cap"])
        assert p.halved_staged >= 0.10 * p.total and p.fallback <= 0.15 * p.total, (name, views, p[:5])
    model = seeded_state(False)
    sd = model.state_dict()
    feats = synth.make_pair_features(N - 1, C, h, w, seed=61)
    t0 = time.time()
    with torch.no_grad():
        want = O.stage_forward(feats, cams, hyp, sd, stage, exact=False)
    print("oracle stage_forward %s: %.1f s" % (name, time.time() - t0))
    model = model.to(dev)
    dfe = [{k2: tuple(t.to(dev) if t is not None else None for t in f[k2]) for k2 in ("ref", "src")} for f in feats]
    with torch.no_grad():
        out = model.stage_net(dfe, cams, depth_values=hyp.to(dev), num_depth=D, cost_regularization=model.cost_regularization[stage],
                              stage_idx=stage)
        ref = torch.stack([f["ref"][0][0] for f in feats]).to(dev).contiguous()
        src = torch.stack([ops.chw_to_hwc(f["src"][0][0].to(dev).contiguous()) for f in feats])
        ref_nc = torch.stack([f["ref"][2][0, 0] for f in feats]).to(dev).contiguous()
        vol, _, _, _ = model.stage_net.aggregate(ref, src, ref_nc, geometry.warp_matrices(cams[0]), hyp[0].to(dev).contiguous(), stage)
    assert torch.isfinite(vol).all()
    assert (vol.cpu() - want["_volume_mean"][0]).abs().max().item() <= 1e-5, name
    assert (out["depth"].cpu() - want["depth"]).abs().mean().item() <= 1e-3, name
    assert (out["photometric_confidence"].cpu() - want["photometric_confidence"]).abs().mean().item() <= 1e-3, name
    assert (out["norm_curv"].cpu() - want["norm_curv"]).abs().max().item() <= 1e-6, name


if __name__ == "__main__":      # the child of test_results_do_not_depend_on_stale_lds
    assert sys.argv[1] == "--child"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cds_mvsnet_amd import ops as _ops
    torch.save(_stale_lds_outputs(sys.argv[2], torch.device("cuda:0"), _ops), sys.argv[3])
