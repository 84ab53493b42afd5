"""The CPU model of the K3 / K1 chunk plan (tests/k3_chunk_plan.py) on hand-checkable cases, and the preconditions of every named input
of tests/test_k3_depth_march_gpu.py - checked here, where no GPU is needed, so a retuned box budget that turns those cases back into
single-path tests is noticed on any machine."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k3_chunk_plan as plan  # noqa: E402
import test_k3_depth_march_gpu as gpu_cases  # noqa: E402  (its case lists; importing it needs no GPU)


def test_constants_are_read_from_the_kernel_source(tmp_path):
    c = plan.kernel_constants()
    assert set(c) == {"K3_TW", "K3_TH", "K3_BOX", "K3_DC", "K1_DC", "K1_BOX"} and all(v > 0 for v in c.values())
    assert c["K3_TW"] * c["K3_TH"] == 256
    assert plan.k1_constants(8)["dc"] == c["K1_DC"] and plan.k1_constants(16) == plan.k3_constants() == plan.k1_constants(32)
    stale = tmp_path / "warp_lds.hip"
    stale.write_text("#define CDS_K3_TW 32\n#define CDS_K3_TH 8\n")
    with pytest.raises(AssertionError, match="CDS_K3_BOX not found"):
        plan.kernel_constants(str(stale))


def test_launcher_segments():
    # D = 145: four 48-plane chunks; few tiles -> one chunk per segment unless CDS_K3_NSEG says otherwise
    assert plan.k3_seg_planes(145, 48, ntiles=15, ngroups=1) == 48
    assert plan.k3_seg_planes(145, 48, 15, 1, nseg_env=1) == 192
    assert plan.k3_seg_planes(145, 48, 15, 1, nseg_env=2) == 96
    assert plan.k3_seg_planes(145, 48, 15, 1, nseg_env=3) == 96       # ceil(4 / 3) = 2 chunks per segment
    assert plan.k3_seg_planes(145, 48, 15, 1, nseg_env=9) == 48
    assert plan.k3_seg_planes(192, 48, ntiles=1280, ngroups=1) == 96   # M1 full size: 5120 < 10240 -> nseg = 2
    assert plan.k3_seg_planes(48, 48, ntiles=495, ngroups=4) == 48
    assert plan.k3_launch_views((1, 2, 3)) == [[1, 2, 3]]
    assert plan.k3_launch_views(range(1, 6)) == [[1, 2, 3], [4, 5]]
    assert plan.k3_launch_views(range(1, 6), 4) == [[1, 2, 3, 4], [5]]
    assert plan.k3_launch_views(range(1, 7), 2) == [[1, 2], [3, 4, 5, 6]]
    assert plan.k3_launch_views(range(1, 8), 3) == [[1, 2, 3], [4, 5, 6, 7]]
    assert plan.k3_launch_views(range(1, 8), 2) == [[1, 2, 3, 4], [5, 6, 7]]   # 2 + 5 is no valid split: the default


def _shear(D, slope, h=8, w=32):
    """One 32x8 tile whose samples move `slope` texels per plane along x: over n planes the box is (w - 1 + slope (n - 1) + 2) x (h + 1)."""
    d = torch.arange(D).view(D, 1, 1)
    cx = (torch.arange(w).view(1, 1, w) + slope * d).expand(D, h, w).contiguous()
    cy = torch.arange(h).view(1, h, 1).expand(D, h, w).contiguous()
    return [(cx, cy)], d.float().expand(D, h, w).contiguous()


def test_known_footprints_give_the_halving_sequence():
    # cap 632, box height 9: a chunk of n planes fits iff 33 + slope (n - 1) <= 70
    cells, hyp = _shear(48, 0)
    assert plan.march(cells, hyp, 48, 632).workgroups == [[(0, 48, True)]]
    # 2 texels / plane: 48 (127 wide) -> 24 (79) -> 12 (55: fits); then 36 left -> 18 (67: fits); then the last 18
    cells, hyp = _shear(48, 2)
    p = plan.march(cells, hyp, 48, 632)
    assert p.workgroups == [[(0, 12, True), (12, 30, True), (30, 48, True)]]
    assert (p.full, p.halved_staged, p.fallback, p.offgrid_starts, p.max_chunks_per_workgroup) == (1, 2, 0, 2, 3)
    # 5 texels / plane (n planes fit iff n <= 8): 48 -> 24 -> 12 -> 6; 42 -> 22 -> 12 -> 6; 36 -> 18 -> 10 -> 6; 30 -> 16 -> 8; 22 -> 12 -> 6;
    # 16 -> 8; the last 8 fit as they are
    bounds = [(0, 6), (6, 12), (12, 18), (18, 26), (26, 32), (32, 40), (40, 48)]
    cells, hyp = _shear(48, 5)
    p = plan.march(cells, hyp, 48, 632)
    assert p.workgroups == [[(a, b, True) for a, b in bounds]]
    assert (p.full, p.halved_staged, p.fallback) == (1, 6, 0) and p.lengths == {6: 4, 8: 3}
    # 12 texels / plane: not even 6 planes fit (93 wide); halving stops at <= 8 planes: the same chunks, all on the global-memory path
    cells, hyp = _shear(48, 12)
    p = plan.march(cells, hyp, 48, 632)
    assert p.workgroups == [[(a, b, False) for a, b in bounds]] and p.fallback == 7
    # K1's C = 8 budget (64 planes, 1016 texels: 33 + slope (n - 1) <= 112) on the 2-texel shear: 64 -> 32 (95: fits)
    cells, hyp = _shear(64, 2)
    assert plan.march(cells, hyp, 64, 1016).workgroups == [[(0, 32, True), (32, 64, True)]]
    # descending hypotheses give the same boxes: the model takes the per-pixel extremes, not the first and last plane
    cells, hyp = _shear(48, 2)
    assert plan.march(cells, -hyp, 48, 632).workgroups == [[(0, 12, True), (12, 30, True), (30, 48, True)]]
    # a plane far away in the MIDDLE of a chunk (non-monotone) widens its box: first / last plane alone would not see it
    cells, hyp = _shear(48, 0)
    cells[0][0][20] += 500
    hyp[20] = 1000.0
    p = plan.march(cells, hyp, 48, 632)
    assert not all(s for _, _, s in p.workgroups[0]) and p.workgroups[0][0] != (0, 48, True)


def test_cells_clamp_like_the_kernel():
    ix = torch.tensor([-7.5, -2.0, -0.5, 3.7, 99.0, float("nan"), float("inf"), float("-inf")])
    cx, cy = plan.cells_of_positions(ix, ix, 10, 20)
    assert cx.tolist() == [-2, -2, -1, 3, 20, -2, 20, -2] and cy.tolist() == [-2, -2, -1, 3, 10, -2, 10, -2]


def test_identity_like_geometry_gives_whole_chunks():
    from cds_mvsnet_amd import synth
    h, w, D = 24, 136, 100
    cams = synth.make_cameras(3, h, w, seed=5, baseline=(0.5, 0.5, 0.1))["stage3"]
    hyp = synth.make_hypotheses(D, h, w, seed=6)
    p = plan.chunk_plan(cams, hyp, [1, 2], 48, 632)
    ntiles = 3 * 5
    assert p.workgroups == [[(0, 48, True), (48, 96, True), (96, 100, True)]] * ntiles
    assert (p.full, p.halved_staged, p.fallback, p.offgrid_starts) == (3 * ntiles, 0, 0, 0)
    p = plan.chunk_plan(cams, hyp, [1], 64, 1016)
    assert p.workgroups == [[(0, 64, True), (64, 100, True)]] * ntiles
    p = plan.chunk_plan(cams, hyp, [1, 2], 48, 632, seg_planes=96)
    assert p.workgroups == [[(0, 48, True), (48, 96, True)], [(96, 100, True)]] * ntiles


@pytest.mark.parametrize("name,D,views,seg_planes,rows", [("B", 145, (1, 2, 3), None, None), ("B", 145, (4, 5, 6), 96, None),
                                                          ("Bperm", 145, (1, 2, 3, 4), 48, None), ("B", 145, (1, 2, 3), None, (13, 43)),
                                                          ("A2", 97, (1, 2, 3, 4), None, None), ("A", 194, (5, 6, 7), 96, (5, 19))])
def test_chunks_tile_the_depth_range(name, D, views, seg_planes, rows):
    cams, hyp = plan.named_input(name, D)
    k = plan.k3_constants()
    p = plan.chunk_plan(cams, hyp, views, k["dc"], k["cap"], seg_planes, rows=rows)
    _, _, h, w = hyp.shape
    y0, y1 = rows or (0, h)
    nseg = -(-D // (seg_planes or D))
    assert len(p.workgroups) == -(-(y1 - y0) // 8) * -(-w // 32) * nseg
    for i in range(0, len(p.workgroups), nseg):       # the segments of one tile, in order
        chunks = [c for wg in p.workgroups[i:i + nseg] for c in wg]
        assert chunks[0][0] == 0 and chunks[-1][1] == D
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))            # no gap, no overlap
        assert all(d0 % 2 == 0 and d1 > d0 and d1 - d0 <= k["dc"] for d0, d1, _ in chunks)
        assert all(staged or d1 - d0 <= 8 for d0, d1, staged in chunks)
    assert p.total == p.full + p.halved_staged + p.fallback


def test_input_b_is_the_one_described():
    """The figures the cases were chosen by (one depth segment): they are properties of the input, so they are pinned here."""
    k = plan.k3_constants()
    p = plan.named_plan("B", 145, (1, 2, 3), k["dc"], k["cap"])
    assert (p.full, p.halved_staged, p.fallback, p.offgrid_starts) == (106, 127, 0, 151) and set(p.lengths) == {48, 37, 25, 24, 13, 12, 6, 1}
    p = plan.named_plan("B", 145, (4, 5, 6), k["dc"], k["cap"])
    assert (p.full, p.halved_staged, p.fallback, p.offgrid_starts) == (110, 103, 14, 147)
    cams, hyp = plan.named_input("B")
    for v in (1, 3, 6):
        assert 0.60 <= plan.in_image_fraction(cams, hyp, v) <= 0.80
    _, hp = plan.named_input("Bperm")
    assert 0.2 < float((hp[:, 1:] < hp[:, :-1]).float().mean()) < 0.5 and torch.equal(hp.sort(1).values, hyp.sort(1).values)


def test_family_a_never_halves_and_marches_long():
    k = plan.k3_constants()
    for name in ("A", "A2"):
        for D in plan.A_DEPTHS:
            for views in ((1, 2, 3, 4), (5, 6, 7)):
                p = plan.named_plan(name, D, views, k["dc"], k["cap"])
                assert p.halved_staged == 0 and p.fallback == 0 and p.max_chunks_per_workgroup == -(-D // k["dc"]) >= 2
    assert set(plan.named_plan("A", 97, (1, 2, 3, 4), 48, 632).lengths) == {48, 1}
    assert set(plan.named_plan("A", 145, (1,), 64, 1016).lengths) == {64, 17} and set(plan.named_plan("A", 97, (1,), 64, 1016).lengths) == {64, 33}


def test_preconditions_of_the_gpu_cases():
    """Every B-family case of test_k3_depth_march_gpu.py asserts these itself on the GPU machine; here they are proven without one."""
    checked = 0
    for name, D, views, C, nseg, cl, exact, normalize in gpu_cases.MARCH_CASES:
        if name.startswith("B"):
            plan.assert_halving_input(name, D, views)
            checked += 1
    for name, D, views, C, nseg, cl, split in gpu_cases.ACC_CASES:
        launches = plan.k3_launch_views(views, split)
        assert len(launches) == 2 and 1 <= len(launches[1]) <= 4 and len(launches[0]) <= 4
        if name.startswith("B"):
            plan.assert_halving_input(name, D, launches[1])
            checked += 1
    assert sorted({len(plan.k3_launch_views(c[2], c[6])[1]) for c in gpu_cases.ACC_CASES}) == [1, 2, 3, 4]
    for name, D, views, C, exact in gpu_cases.K1_CASES:
        if name.startswith("B"):
            plan.assert_k1_halving_input(name, D, views, C)
            checked += 1
    plan.assert_halving_input("B", 145, (3, 4))          # the accumulating call of the 2 + 2 case
    assert checked >= 25
    # every view count, every C, both layouts, both position modes, all three segment settings appear in the march cases
    assert {len(c[2]) for c in gpu_cases.MARCH_CASES} == {1, 2, 3, 4} and {c[3] for c in gpu_cases.MARCH_CASES} == {8, 16, 32}
    assert {c[4] for c in gpu_cases.MARCH_CASES} == {None, 1, 2} and {c[1] for c in gpu_cases.MARCH_CASES if c[0] == "A"} == set(plan.A_DEPTHS)
    # the samples of every B view used are mostly inside the source image (the GPU cases assert the oracle's non-zero share)
    cams, hyp = plan.named_input("B")
    assert all(plan.in_image_fraction(cams, hyp, v) >= 0.60 for v in range(1, 8))


def test_input_w_is_wild_and_hits_the_image():
    """The preconditions of test_k3_k1_wild_geometry_w_vs_oracle, proven without a GPU: (nearly) all chunks on the global-memory path,
    the samples still inside the source images, and an oracle volume with content."""
    frac = plan.assert_wild_input()
    assert 0.70 <= frac[0] <= 0.76 and 0.73 <= frac[1] <= 0.79 and 0.07 <= frac[2] <= 0.11, frac     # the figures the input was chosen by
    k = plan.k3_constants()
    D = plan.W_SHAPE[1]
    p = plan.named_plan("W", D, (1, 2, 3), k["dc"], k["cap"])
    assert p.fallback == p.total == 150
    p = plan.named_plan("W", D, (1, 2), k["dc"], k["cap"])
    assert p.fallback >= 0.9 * p.total and p.total >= 100
    for C, share in ((8, 0.6), (16, 0.85)):
        kk = plan.k1_constants(C)
        p = plan.merge([plan.named_plan("W", D, [v], kk["dc"], kk["cap"]) for v in (1, 2, 3)])
        assert p.fallback >= share * p.total, (C, p[:5])
    cams, hyp = plan.named_input("W", D)
    # unordered per pixel: about half of the neighbouring plane pairs descend
    assert 0.4 < float((hyp[:, 1:] < hyp[:, :-1]).float().mean()) < 0.6
    assert gpu_cases.w_oracle_content(8) >= 0.5
    want, _ = gpu_cases._oracle_volume("W", D, 8, gpu_cases.W_VIEWS, normalize=False)
    assert float(torch.isfinite(want).float().mean()) >= 0.99
    assert all(torch.isfinite(gpu_cases._oracle_view("W", D, 8, v)[1]).float().mean() >= 0.99 for v in gpu_cases.W_VIEWS)


def test_old_wild_input_has_no_sample_inside_any_image():
    """What test_warp_lds_fallbacks_wild_geometry (test_hip_parity.py) really is: with its baseline and depths no sample of any view
    has even one tap inside the source image, so its expected volume is identically zero."""
    from cds_mvsnet_amd import synth
    V, D, h, w = 3, 40, 24, 136
    cams = synth.make_cameras(V + 1, h, w, refine=False, seed=91, baseline=(900.0, 300.0, 40.0))["stage3"]
    cams[0, 3, 0, :3, 3] += torch.tensor([0.0, 0.0, -260.0])
    hyp = 120.0 + 600.0 * torch.rand(1, D, h, w, generator=torch.Generator().manual_seed(91))
    for v in range(1, V + 1):
        assert plan.in_image_fraction(cams, hyp, v) == 0.0
        cx, cy = plan.sample_cells(cams, hyp, v)          # a tap inside needs a cell in [-1, n - 1]
        assert not bool(((cx >= -1) & (cx <= w - 1) & (cy >= -1) & (cy <= h - 1)).any())


def test_config4_stage1_meets_halved_chunks():
    k = plan.k3_constants()
    for name in ("cfg4", "cfg4near"):
        for views in plan.k3_launch_views(range(1, 7)):
            p = plan.named_plan(name, 48, views, k["dc"], k["cap"])
            assert p.halved_staged >= 0.10 * p.total and p.fallback <= 0.15 * p.total, (name, views, p[:5])
