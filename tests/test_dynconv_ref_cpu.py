"""tests/dynconv_ref.py is sound and sharp (no GPU): PyTorch's own fp32 evaluation of the DynamicConv stays inside HALF the bound on
every case the GPU test runs, the bound says something at almost every pixel, and thirteen one-line defects - each a way a kernel's
epilogue, slot map or operand staging could be wrong - fall outside it."""
import collections

import pytest
import torch

import dynconv_ref as D

F64 = torch.float64
FAMILIES = {"blend": (D.BLEND_CASES, D.blend_case), "fused_sbf": (D.FUSED_CASES, D.fused_case), "dynconv_cl": (D.CL_CASES, D.cl_case),
            "conv00_cl": (D.CONV00_CASES, D.conv00_case)}


def test_the_case_lists_cover_what_they_claim():
    assert {p[5] for p in D.BLEND_CASES} == {1, 2, D.BLEND_N}
    for K in (2, 3):
        assert {p[5] for p in D.BLEND_CASES if p[0] == K} == {1, 2, D.BLEND_N}
    for hw in D.BLEND_SIZES:
        assert {p[5] for p in D.BLEND_CASES if p[2:4] == hw} == {1, 2, D.BLEND_N}
    assert sorted(h * w for h, w in D.BLEND_SIZES) == [1, 1023, 1024, 1025, 1300]
    assert {p[5] for p in D.BLEND_CASES if p[:2] == (3, 8)} == {1, 2, D.BLEND_N}            # what dynconv_blend_cl supports
    assert all(W % 4 == 0 for _, _, _, W, _ in D.FUSED_CASES)
    kinds = D.epipoles(5, 9, 36)
    assert kinds[1].tolist() == [18.0, 3.0] and kinds[3].tolist() == [-0.5, 8.5] and kinds[4].tolist() == [1e6, -3e7]
    assert 0 < kinds[2, 0] < 35 and 0 < kinds[2, 1] < 8 and kinds[2, 0] % 1 and kinds[2, 1] % 1      # sub-pixel, inside
    seen = collections.defaultdict(set)
    for fam, _, case in D.all_cases():                    # w2 is not zero, bias on the response channels only, scales of both signs
        assert case["w2"].abs().min() > 0
        if case.get("bias") is not None:
            assert (case["bias"][:, -3:] == 0).all() and case["bias"][:, :-3].abs().min() > 0
        if case.get("in_affine") is not None:
            assert (case["in_affine"][..., 0] < 0).any() and (case["in_affine"][..., 0] > 0).any()
        H, W = (case["branches"] if "branches" in case else case["x"]).shape[-2:]
        kinds = D.epipoles(5, H, W)
        seen[fam] |= {i for e in case["epi"] for i in range(5) if torch.equal(e, kinds[i])}
    assert all(seen[fam] == {0, 1, 2, 3, 4} for fam in FAMILIES), dict(seen)      # every epipole kind meets every family


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_fp32_torch_stays_inside_half_the_bound_and_few_pixels_are_loose(family):
    """Every case x temperature of the GPU test: |torch fp32 - float64| <= 0.5 x bound at every pixel (the measurement C_CONV and C_CHAIN
    come from), and the loose-pixel caps: per case of >= LOOSE_MIN_PIXELS pixels and over the whole family."""
    params, make = FAMILIES[family]
    loose, pixels = collections.Counter(), collections.Counter()
    for p in params:
        case = make(*p)
        for T in D.TEMPS:
            r64, b = D.ref_and_bound(case, T)
            r32, _ = D.ref_and_bound(case, T, torch.float32)
            share = D.check(r32["out"], r32["norm_curv"], r64, b, f"torch fp32 {family}", limit=0.5)
            n = r64["norm_curv"].numel()
            loose[T] += round(share * n)
            pixels[T] += n
            if n >= D.LOOSE_MIN_PIXELS:
                assert share <= D.LOOSE_CAP[T], (family, p, T, share)
    for T in D.TEMPS:
        print(f"{family} T = {T}: {loose[T]} of {pixels[T]} pixels loose")
        assert loose[T] <= D.LOOSE_CAP[T] * pixels[T], (family, T, loose[T], pixels[T])
    print(f"{family}: worst torch fp32 ratio {D.RATIOS[f'torch fp32 {family}']:.3f}")
    assert D.RATIOS[f"torch fp32 {family}"] <= 0.5


def test_float64_reference_agrees_with_the_training_restatement():
    """reference() against tests/torch_training_ref.py::dynamic_conv (the float64 restatement the training kernels are held to) on a
    module with the same weights: the two were written apart, from models/dynamic_conv.py:97-122."""
    import torch.nn as nn
    import torch_training_ref as R
    case = D.make_conv_case(7, 8, 8, (3, 5, 7), 3, 1, 9, 14, False, True, epi_start=2)
    K = 3

    class DC(nn.Module):
        def __init__(self):
            super().__init__()
            self.att_convs = nn.ModuleList([nn.Conv2d(8, 3, k, padding=(k - 1) // 2, bias=False) for k in (3, 5, 7)])
            self.convs = nn.ModuleList([nn.Conv2d(8, 8, k, padding=(k - 1) // 2) for k in (3, 5, 7)])
            self.fc1, self.fc2 = nn.Conv2d(K, 4, 1), nn.Conv2d(4, K, 1, bias=False)

        def att_weights(self, c):
            return self.fc2(torch.relu(self.fc1(c)))

    dc = DC().double()
    with torch.no_grad():
        for i in range(K):
            dc.convs[i].weight.copy_(case["ws"][i][:8])
            dc.convs[i].bias.copy_(case["bias"][i][:8])
            dc.att_convs[i].weight.copy_(case["ws"][i][8:])
        dc.fc1.weight.copy_(case["w1"].reshape(4, K, 1, 1))
        dc.fc1.bias.copy_(case["b1"])
        dc.fc2.weight.copy_(case["w2"].reshape(K, 4, 1, 1))
        for T in (1.0, 0.01):
            out, nc = R.dynamic_conv(dc, case["x"].double(), case["epi"].double(), T)
            r64, b = D.ref_and_bound(case, T)
            # the training restatement builds its pixel grid in float32 and subtracts the epipole there: same values for these epipoles
            assert D.check(out.float(), nc[:, 0].float(), r64, b, "torch_training_ref") >= 0.0


# ------------------------------------------------------------------------------------------------
# mutants: the float64 reference with ONE defect in place of a kernel's output must fail check()
# ------------------------------------------------------------------------------------------------
def _conv_case():
    """8 -> 8, kernel sizes 3 / 5 / 7, 9 x 36 (not square), bias, pending affine with negative scales, epipoles: outside, on a pixel
    centre, sub-pixel inside."""
    return D.make_conv_case(11, 8, 8, (3, 5, 7), 3, 1, 9, 36, True, True, epi_start=0)


def _shared_case():
    return D.make_blend_case(12, 3, 8, 5, 2, 9, 36, epi_start=0)


def _reblend(r, case, T, basis=None, w1=None, b1=None, w2=None, relu=True):
    basis = r["basis"] if basis is None else basis
    w1, b1, w2 = (case[k].double() if v is None else v for k, v in (("w1", w1), ("b1", b1), ("w2", w2)))
    if relu:
        m = D.blend(r["att"], r["res"], basis, w1, b1, w2, T)
        return m["out"], m["norm_curv"]
    curv = (r["att"] * basis[:, None]).sum(2)
    z = torch.einsum("kj,njhw->nkhw", w2, torch.einsum("jk,nkhw->njhw", w1, curv) + b1[None, :, None, None])
    wt = torch.softmax(z / T, dim=1)
    return (r["res"] * wt[:, :, None]).sum(1), (curv * wt).sum(1)


def _again(case, T, **changed):
    r = D.ref_and_bound({**case, **changed}, T)[0]
    return r["out"], r["norm_curv"]


def _mutant(name, case, r, T):
    K = case["w1"].shape[1]
    N, _, H, W = r["out"].shape
    if name == "epipole x and y swapped":
        return _again(case, T, epi=case["epi"][:, [1, 0]].contiguous())
    if name == "2uv without the 2":
        b = r["basis"].clone()
        b[:, 1] /= 2
        return _reblend(r, case, T, basis=b)
    if name == "+1e-6 dropped (epipole on a pixel centre)":
        return _reblend(r, case, T, basis=D.epipolar_basis(case["epi"], H, W, F64, eps=0.0))
    if name == "w1 indexed [k*4+j]":
        return _reblend(r, case, T, w1=case["w1"].double().reshape(-1).reshape(K, 4).t())
    if name == "w2 transposed":
        return _reblend(r, case, T, w2=case["w2"].double().reshape(-1).reshape(4, K).t())
    if name == "ReLU missing":
        return _reblend(r, case, T, relu=False)
    if name == "b1 missing":
        return _reblend(r, case, T, b1=torch.zeros(4, dtype=F64))
    if name == "division by T missing":
        return _reblend(r, case, 1.0)
    if name == "norm_curv weighted with the logits":
        return r["out"], (r["curv"] * r["z"] / T).sum(1)
    if name == "slot mapping off by one":
        ns = case["n_shared"]
        br = case["branches"].double()[:, [0 if n < ns else n - ns for n in range(N)]].transpose(0, 1)
        m = D.blend(br[:, :, -3:], br[:, :, :-3], r["basis"], case["w1"].double(), case["b1"].double(), case["w2"].double(), T)
        return m["out"], m["norm_curv"]
    if name == "x / y from p % H":
        p = torch.arange(H * W)
        xs, ys = (p % H).double().reshape(1, H, W), (p // H).double().reshape(1, H, W)
        u, v = xs - case["epi"][:, 0, None, None].double(), ys - case["epi"][:, 1, None, None].double()
        nrm = torch.sqrt(u * u + v * v)
        u, v = u / (nrm + 1e-6), v / (nrm + 1e-6)
        return _reblend(r, case, T, basis=torch.stack((u * u, 2 * u * v, v * v), 1))
    if name == "LeakyReLU slope ignored":
        a = case["in_affine"].clone()
        a[..., 2] = 1.0
        return _again(case, T, in_affine=a)
    if name == "bias of one branch dropped":
        b = case["bias"].clone()
        b[1] = 0.0
        return _again(case, T, bias=b)
    raise KeyError(name)


MUTANTS = ["epipole x and y swapped", "2uv without the 2", "+1e-6 dropped (epipole on a pixel centre)", "w1 indexed [k*4+j]", "w2 transposed",
           "ReLU missing", "b1 missing", "division by T missing", "norm_curv weighted with the logits", "slot mapping off by one",
           "x / y from p % H", "LeakyReLU slope ignored", "bias of one branch dropped"]


@pytest.mark.parametrize("name", MUTANTS)
def test_mutants_are_rejected(name):
    """At every temperature (but T = 1 for the missing division, which changes nothing there), on a convolving case and on a
    shared-slot blend case where the defect applies: check() raises.  The unmutated float64 reference passes with ratio 0."""
    for case in (_shared_case(),) if name == "slot mapping off by one" else (_conv_case(), _shared_case()):
        if name in ("LeakyReLU slope ignored", "bias of one branch dropped") and "branches" in case:
            continue
        for T in D.TEMPS:
            if name == "division by T missing" and T == 1.0:
                continue
            r64, b = D.ref_and_bound(case, T)
            D.check(r64["out"], r64["norm_curv"], r64, b, "float64 reference")
            out, nc = _mutant(name, case, r64, T)
            with pytest.raises(AssertionError):
                D.check(out, nc, r64, b, f"mutant: {name}")
    assert D.RATIOS["float64 reference"] == 0.0


def test_check_stats_accepts_the_truth_and_rejects_a_dropped_pixel():
    g = torch.Generator().manual_seed(5)
    out = torch.randn(2, 8, 9, 13, generator=g) * 2.0 + 0.5
    y = out.double()
    s, q = y.sum((2, 3)), (y * y).sum((2, 3))
    mean = s / 117
    inv = 1.0 / torch.sqrt(q / 117 - mean * mean + 1e-5)
    aff = torch.stack((inv, -mean * inv, torch.full_like(inv, 0.1)), -1).float()
    D.check_stats(out, torch.stack((s, q), -1), aff, 0.1, "truth")
    with pytest.raises(AssertionError):
        D.check_stats(out, torch.stack((s - y[:, :, -1, -1], q), -1), aff, 0.1, "last pixel missing from the sum")
    with pytest.raises(AssertionError):
        D.check_stats(out, torch.stack((s, q), -1), aff, 0.01, "another slope")
