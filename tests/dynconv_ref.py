"""Float64 restatement of the inference DynamicConv (models/dynamic_conv.py:97-122), an a-priori error bound for an fp32
implementation of it, the checker that holds a kernel to that bound, and the cases both test files run.  CPU torch only, nothing of the
library under test.  tests/test_dynconv_ref_cpu.py shows that the checker is sound (PyTorch's own fp32 evaluation passes with room) and
sharp (thirteen one-line defects fail); tests/test_dynconv_f64_gpu.py holds the HIP kernels to it.

  reference()   out, norm_curv and every intermediate in a given dtype: float64 is the reference, float32 is "torch's own fp32
                evaluation of the same expression", the unit the constants below are measured in
  bound()       per-pixel bound on |fp32 implementation - float64| from the float64 magnitudes
  check()       finite, inside the bound at EVERY pixel; returns the share of pixels whose bound says little

The bound (u = 2^-24; every sum below is over float64 magnitudes, so it is a property of the data, not of an implementation):
  e_br   = u (conv2d(c_conv |x| + 2 m, |w|) + c_conv |bias|)                    a branch response; 0 when the branch tensor is the input.
                                                                                x: the input AFTER its pending affine; m = |x0 a| + |b|
                                                                                with a pending affine (its own two roundings, which
                                                                                scale with the terms, not with their sum), else 0
  e_curv = sum_j e_att_j |basis_j| + c_chain u sum_j |att_j| |basis_j|          the projection onto [u^2, 2uv, v^2] (|basis_j| <= 1)
  e_hid  = sum_k |w1_jk| e_curv_k + c_chain u (sum_k |w1_jk| |curv_k| + |b1_j|)  ReLU is 1-Lipschitz; and 0 where the unit is off by more
                                                                                than this (w1 curv + b1 < -e_hid): it stays exactly 0
  e_z    = sum_j |w2_kj| e_hid_j + c_chain u sum_j |w2_kj| |hid_j|
  delta  = max_k e_z / T + c_chain u (max |z| / T + 1)                          the logits as softmax sees them (+ the exp's own rounding)
  dw_k   = min(w_k, 1 - w_k) expm1(2 delta), at most 1                          see below
  e_out  = max_k e_res_k + sum_k dw_k |res_k - out| + c_chain u max_k |res_k| + u max(1, max |out|)
  e_nc   = the same with curv in place of res.
dw: moving every logit by at most delta multiplies w_k / (1 - w_k) by a factor in [e^-2delta, e^2delta], so
|w_k' - w_k| <= w_k (1 - w_k) expm1(2 delta) / (1 + w_k expm1(2 delta)) <= min(w_k, 1 - w_k) expm1(2 delta).  The plain Lipschitz bound
delta / 2 ignores that a saturated softmax does not move: at T <= 0.01 it leaves most pixels with a bound above 1e-3 and the test
would say nothing there.  sum_k dw_k (res_k - out) is the first-order change of out because sum_k dw_k = 0.

Constants.  c_conv and c_chain are the smallest powers of two at which PyTorch's fp32 evaluation of reference() on the CPU stays at or
below HALF the bound at every pixel of every case of both test files (all_cases(), every temperature):
  c_conv = 8, c_chain = 8.  Measured worst ratio |torch fp32 - float64| / bound per family (test_dynconv_ref_cpu.py asserts <= 0.5):
      (c_conv, c_chain)   blend   fused_sbf   dynconv_cl   conv00_cl
      (8, 8)  chosen      0.425   0.403       0.379        0.330
      (4, 8)              0.425   0.735       0.520        0.543          c_conv too small
      (8, 4)              0.784   0.450       0.401        0.365          c_chain too small
      (4, 4)              0.784   0.773       0.562        0.631
  The worst pixels: blend - norm_curv next to an epipole on a pixel centre (T = 1); fused_sbf - 16 channels, kernel sizes 3 / 5 / 7 (the
  longest sums: PyTorch's CPU convolution rounds in its own blocked order).
The kernels are allowed ratio 1.0: twice what PyTorch's fp32 needs, in line with the "<= 1.5 x the fp32 error + one ulp" rule of the
split-bf16 / split-f16 layers.

Loose pixels.  A pixel whose bound exceeds 1e-3 max(1, max |out|) is "loose": softmax(./T) amplifies there (two logits within a few
delta of each other) and any fp32 implementation may land on either side.  The MLP scales of the cases (MLP_SCALE: a second layer of
standard deviation 8 separates the logits) are chosen so that loose pixels are rare: test_dynconv_ref_cpu.py asserts <= 1 % for
T >= 0.01 and <= 10 % at T = 0.001 over every kernel family, and for every single case of at least LOOSE_MIN_PIXELS pixels (one loose
pixel of a 1 x 1 image is 100 %: a share means nothing there).  Measured: at most 0.24 % of a family's pixels (conv00_cl, T = 0.01) and
0.59 % of a single case.  Without the ReLU term of e_hid the 7 % of pixels whose four hidden units are all off (logits exactly equal,
weights exactly 1 / K in any implementation) were all loose.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
C_CONV = 8.0
C_CHAIN = 8.0
TEMPS = (1.0, 0.01, 0.001)
LOOSE_REL = 1e-3
LOOSE_CAP = {1.0: 0.01, 0.01: 0.01, 0.001: 0.10}
LOOSE_MIN_PIXELS = 1000
MLP_SCALE = (1.0, 1.0, 8.0)          # standard deviations of w1, b1, w2

RATIOS = {}                           # check(): worst ratio per name, for the summaries the tests print


# ------------------------------------------------------------------------------------------------
# the operation
# ------------------------------------------------------------------------------------------------
def slot_of(N, n_shared):
    """Image n reads slot 0 if n < n_shared else n - n_shared + 1."""
    return torch.tensor([0 if n < n_shared else n - n_shared + 1 for n in range(N)], dtype=torch.long)


def post_affine(x, in_affine, dtype):
    """x [S,C,H,W] after its pending affine (scale, shift, LeakyReLU slope) in ``dtype``; in_affine [S,C,3] or None."""
    y = x.to(dtype)
    if in_affine is None:
        return y
    a = in_affine.to(dtype)
    y = y * a[:, :, 0, None, None] + a[:, :, 1, None, None]
    return torch.where(y > 0, y, y * a[:, :, 2, None, None])


def epipolar_basis(epi, H, W, dtype, eps=1e-6):
    """[u^2, 2uv, v^2] of the unit direction from the epipole: epi [N,2] (x, y) -> [N,3,H,W] (dynamic_conv.py:100-107,113)."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    e = epi.to(dtype)
    u = xs[None] - e[:, 0, None, None]
    v = ys[None] - e[:, 1, None, None]
    nrm = torch.sqrt(u ** 2 + v ** 2)
    u, v = u / (nrm + eps), v / (nrm + eps)
    return torch.stack((u ** 2, 2 * u * v, v ** 2), dim=1)


def blend(att, res, basis, w1, b1, w2, T):
    """att [N,K,3,H,W], res [N,K,C,H,W], basis [N,3,H,W]; the 1x1 MLP w1 [4,K], b1 [4] (BatchNorm folded), w2 [K,4] ->
    dict(out [N,C,H,W], norm_curv [N,H,W], curv [N,K,H,W], hid [N,4,H,W], z [N,K,H,W], wt [N,K,H,W])  (dynamic_conv.py:113-121)."""
    dtype = att.dtype
    curv = (att * basis[:, None]).sum(dim=2)
    hid = torch.relu(torch.einsum("jk,nkhw->njhw", w1.to(dtype), curv) + b1.to(dtype)[None, :, None, None])
    z = torch.einsum("kj,njhw->nkhw", w2.to(dtype), hid)
    wt = torch.softmax(z / T, dim=1)
    return {"out": (res * wt[:, :, None]).sum(dim=1), "norm_curv": (curv * wt).sum(dim=1), "curv": curv, "hid": hid, "z": z, "wt": wt}


def reference(x, in_affine, ws, bias, w1, b1, w2, epi, T, n_shared, dtype, branches=None):
    """The inference DynamicConv in ``dtype``.  x [S,Cin,H,W] (S = N - n_shared + 1 slots) with its pending affine in_affine [S,Cin,3]
    or None; ws: per kernel size [Cout + 3, Cin, k, k] (convs[k] then att_convs[k]); bias [K,Cout + 3] or None; epi [N,2].
    branches [K,S,Cout + 3,H,W] given: the branch responses themselves (x, in_affine, ws and bias are not read).
    -> dict: out, norm_curv, att, res, basis, curv, hid, z, wt (per IMAGE, through the slot map), x_post (per slot; None with branches)."""
    N = epi.shape[0]
    xp = None
    if branches is None:
        xp = post_affine(x, in_affine, dtype)
        br = torch.stack([F.conv2d(xp, w.to(dtype), None if bias is None else bias[i].to(dtype), padding=(w.shape[-1] - 1) // 2)
                          for i, w in enumerate(ws)])
    else:
        br = branches.to(dtype)
    K, S, C3, H, W = br.shape
    assert S == N - n_shared + 1, (S, N, n_shared)
    br = br[:, slot_of(N, n_shared)].transpose(0, 1)                # [N,K,C3,H,W]
    att, res = br[:, :, C3 - 3:], br[:, :, :C3 - 3]
    basis = epipolar_basis(epi, H, W, dtype)
    r = blend(att, res, basis, w1, b1, w2, T)
    r.update(att=att, res=res, basis=basis, x_post=xp, x_mag=None)
    if branches is None and in_affine is not None:                  # |x a| + |b|: what the rounding of the affine itself scales with
        a = in_affine.to(dtype).abs()
        r["x_mag"] = x.to(dtype).abs() * a[:, :, 0, None, None] + a[:, :, 1, None, None]
    return r


# ------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------
def bound(ref64, w1, b1, w2, T, n_shared, ws=None, bias=None, c_conv=C_CONV, c_chain=C_CHAIN):
    """Per-pixel bound on |fp32 implementation - float64| (module docstring) from the float64 intermediates ``ref64`` of reference().
    ws (and bias) given: the branches were convolved from ref64["x_post"]; ws None: the branch tensor was the input, e_br = 0.
    -> dict(out [N,C,H,W], norm_curv [N,H,W])."""
    att, res, basis, curv, hid, z, wt = (ref64[k] for k in ("att", "res", "basis", "curv", "hid", "z", "wt"))
    N, K, C = res.shape[:3]
    f = torch.float64
    if ws is not None:
        xa = ref64["x_post"].abs() * c_conv
        if ref64["x_mag"] is not None:
            xa = xa + 2.0 * ref64["x_mag"]
        e_br = torch.stack([F.conv2d(xa, w.to(f).abs(), None if bias is None else c_conv * bias[i].to(f).abs(), padding=(w.shape[-1] - 1) // 2)
                            for i, w in enumerate(ws)]) * U
        e_br = e_br[:, slot_of(N, n_shared)].transpose(0, 1)
        e_att, e_res = e_br[:, :, C:], e_br[:, :, :C]
    else:
        e_att, e_res = torch.zeros_like(att), torch.zeros_like(res)
    ab = basis.abs()[:, None]
    e_curv = (e_att * ab).sum(2) + c_chain * U * (att.abs() * ab).sum(2)
    a1, a2 = w1.to(f).abs(), w2.to(f).abs()
    e_hid = torch.einsum("jk,nkhw->njhw", a1, e_curv) + c_chain * U * (torch.einsum("jk,nkhw->njhw", a1, curv.abs())
                                                                       + b1.to(f).abs()[None, :, None, None])
    pre = torch.einsum("jk,nkhw->njhw", w1.to(f), curv) + b1.to(f)[None, :, None, None]
    e_hid = torch.where(pre < -e_hid, torch.zeros_like(e_hid), e_hid)       # a unit that is off by more than its error is exactly 0
    e_z = torch.einsum("kj,njhw->nkhw", a2, e_hid) + c_chain * U * torch.einsum("kj,njhw->nkhw", a2, hid.abs())
    delta = e_z.amax(1) / T + c_chain * U * (z.abs().amax(1) / T + 1.0)
    dw = (torch.minimum(wt, 1.0 - wt) * torch.expm1(2.0 * delta)[:, None]).clamp(max=1.0)                 # [N,K,H,W]
    out, nc = ref64["out"], ref64["norm_curv"]
    e_out = (e_res.amax(1) + (dw[:, :, None] * (res - out[:, None]).abs()).sum(1) + c_chain * U * res.abs().amax(1)
             + U * max(1.0, out.abs().max().item()))
    e_nc = (e_curv.amax(1) + (dw * (curv - nc[:, None]).abs()).sum(1) + c_chain * U * curv.abs().amax(1)
            + U * max(1.0, nc.abs().max().item()))
    return {"out": e_out, "norm_curv": e_nc}


def loose_mask(ref64, bounds):
    """[N,H,W] bool: the bound of a channel of ``out`` or of ``norm_curv`` exceeds 1e-3 max(1, max |.|) at this pixel."""
    so, sn = max(1.0, ref64["out"].abs().max().item()), max(1.0, ref64["norm_curv"].abs().max().item())
    return (bounds["out"].amax(1) > LOOSE_REL * so) | (bounds["norm_curv"] > LOOSE_REL * sn)


def check(got_out, got_nc, ref64, bounds, name, limit=1.0):
    """got_out [N,C,H,W] / got_nc [N,H,W] (CPU tensors of an fp32 implementation) against reference(..., float64) and bound(): finite,
    and |got - ref64| <= limit x bound at EVERY pixel.  Prints the worst ratio (kept in RATIOS[name]); -> the share of loose pixels."""
    assert got_out.shape == ref64["out"].shape and got_nc.shape == ref64["norm_curv"].shape, (name, got_out.shape, got_nc.shape)
    assert torch.isfinite(got_out).all() and torch.isfinite(got_nc).all(), (name, "non-finite output")
    worst = 0.0
    for what, got in (("out", got_out), ("norm_curv", got_nc)):
        err = (got.double() - ref64[what]).abs()
        assert torch.isfinite(bounds[what]).all() and (bounds[what] > 0).all(), (name, what, "the bound itself is not finite and positive")
        ratio = err / bounds[what]
        i = int(ratio.argmax())
        r = ratio.reshape(-1)[i].item()
        worst = max(worst, r)
        assert r <= limit, (name, what, f"|got - float64| = {err.reshape(-1)[i].item():.3e} > {limit} x bound {bounds[what].reshape(-1)[i].item():.3e} "
                                        f"at flat index {i} of {tuple(got.shape)}; {int((ratio > limit).sum())} elements outside")
    loose = loose_mask(ref64, bounds).double().mean().item()
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
    print(f"{name}: worst |got - float64| / bound = {worst:.3f}, loose pixels {100.0 * loose:.2f} %")
    return loose


def check_stats(out, stats, affine, slope, name):
    """The statistics a kernel leaves next to its output ``out`` [N,C,H,W] (CPU): stats [N,C,2] float64 = (sum, sum of squares) of the
    kernel's OWN output, affine [N,C,3] = (1 / sqrt(var + 1e-5), -mean / sqrt(var + 1e-5), slope), both recomputed here in float64."""
    y = out.double()
    hw = y.shape[2] * y.shape[3]
    s, q = y.sum((2, 3)), (y * y).sum((2, 3))
    assert stats.dtype == torch.float64 and affine.dtype == torch.float32
    assert torch.allclose(stats[..., 0], s, rtol=1e-10, atol=1e-7), (name, "sum", (stats[..., 0] - s).abs().max().item())
    assert torch.allclose(stats[..., 1], q, rtol=1e-10, atol=1e-7), (name, "sum of squares", (stats[..., 1] - q).abs().max().item())
    mean = s / hw
    inv = 1.0 / torch.sqrt((q / hw - mean * mean).clamp_min(0.0) + 1e-5)
    want = torch.stack((inv, -mean * inv, torch.full_like(inv, slope)), dim=-1)
    assert torch.allclose(affine.double(), want, rtol=1e-5, atol=1e-6), (name, "affine", (affine.double() - want).abs().max().item())


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def epipoles(N, H, W, start=0):
    """One epipole per image, cycling from kind ``start`` through: outside the image (as the older tests place it); exactly on a pixel
    centre inside (u = v = 0 there); sub-pixel inside; on the half-pixel border (-0.5, H - 0.5); far away (1e6, -3e7)."""
    kinds = ((W * 0.3 + 5.0, -H * 1.7 - 1.0), (float(W // 2), float(H // 3)), (W * 0.537 - 0.13, H * 0.321 + 0.21), (-0.5, H - 0.5),
             (1e6, -3e7))
    return torch.tensor([kinds[(start + n) % 5] for n in range(N)], dtype=torch.float32)


def mlp(K, g):
    s1, sb, s2 = MLP_SCALE
    return torch.randn(4, K, generator=g) * s1, torch.randn(4, generator=g) * sb, torch.randn(K, 4, generator=g) * s2       # w2 is NOT zero


def affine_table(S, C, g):
    """(scale, shift, slope 0.1) rows with scales of both signs: a negative scale sends the positive half of the input through the
    LeakyReLU branch."""
    scale = (0.5 + torch.rand(S, C, generator=g)) * torch.where(torch.rand(S, C, generator=g) < 0.4, -1.0, 1.0)
    return torch.stack((scale, 0.3 * torch.randn(S, C, generator=g), torch.full((S, C), 0.1)), dim=-1).contiguous()


def conv_weights(cin, cout, ks, g):
    """Per kernel size [cout + 3, cin, k, k]: response channels ~ 1 / sqrt(fan-in), curvature channels std 0.1 (dynamic_conv.py:95)."""
    return [torch.cat((torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, torch.randn(3, cin, k, k, generator=g) * 0.1)).contiguous()
            for k in ks]


def branch_bias(K, cout, g):
    b = torch.randn(K, cout + 3, generator=g)
    b[:, cout:] = 0.0                        # the att convolutions have no bias (dynamic_conv.py:86)
    return b


def make_conv_case(seed, cin, cout, ks, S, n_shared, H, W, affine, bias, image=False, epi_start=0):
    """Inputs of one convolving case as a dict of CPU float32 tensors (the keyword arguments of reference() but T and dtype)."""
    g = torch.Generator().manual_seed(seed)
    N = S + n_shared - 1
    x = torch.rand(S, cin, H, W, generator=g) if image else torch.randn(S, cin, H, W, generator=g)
    w1, b1, w2 = mlp(len(ks), g)
    return {"x": x, "in_affine": affine_table(S, cin, g) if affine else None, "ws": conv_weights(cin, cout, ks, g),
            "bias": branch_bias(len(ks), cout, g) if bias else None, "w1": w1, "b1": b1, "w2": w2, "epi": epipoles(N, H, W, epi_start),
            "n_shared": n_shared}


def make_blend_case(seed, K, cout, N, n_shared, H, W, epi_start=0):
    """Inputs of one blend-only case: an exact branch tensor [K,S,cout + 3,H,W] (response channels ~ N(0, 1), curvature ~ N(0, 0.5^2))."""
    g = torch.Generator().manual_seed(seed)
    S = N - n_shared + 1
    br = torch.randn(K, S, cout + 3, H, W, generator=g)
    br[:, :, cout:] *= 0.5
    w1, b1, w2 = mlp(K, g)
    return {"branches": br.contiguous(), "w1": w1, "b1": b1, "w2": w2, "epi": epipoles(N, H, W, epi_start), "n_shared": n_shared}


def ref_and_bound(case, T, dtype=torch.float64, ref64=None):
    """-> (reference(case) in dtype, bound from the float64 reference or None for another dtype)."""
    kw = dict(w1=case["w1"], b1=case["b1"], w2=case["w2"], epi=case["epi"], T=T, n_shared=case["n_shared"], dtype=dtype)
    if "branches" in case:
        r = reference(None, None, None, None, branches=case["branches"], **kw)
    else:
        r = reference(case["x"], case["in_affine"], case["ws"], case["bias"], **kw)
    if dtype != torch.float64:
        return r, None
    return r, bound(r, case["w1"], case["b1"], case["w2"], T, case["n_shared"], ws=case.get("ws"), bias=case.get("bias"))


# blend kernels: H W = 1, 1023, 1024, 1025 sit either side of the 4-pixels-per-thread, 256-thread block; one 13 x 100 image
BLEND_SIZES = ((1, 1), (31, 33), (32, 32), (25, 41), (13, 100))
BLEND_KC = tuple((K, c) for K in (2, 3) for c in (8, 11, 16, 32))
BLEND_N = 5
# (K, cout, H, W, N, n_shared): every (K, cout) at every size; n_shared in {1, 2, N} rotates so that every K, every cout and every size
# meets each of the three
BLEND_CASES = tuple((K, c, H, W, BLEND_N, (1, 2, BLEND_N)[(i + j) % 3]) for i, (K, c) in enumerate(BLEND_KC) for j, (H, W) in enumerate(BLEND_SIZES))

# planar fused kernel (W % 4 == 0): the five DynamicConv shapes of FeatureNet past conv00 and (16, (3, 5, 7)), the one instantiation
# (three branches, two 16-column blocks) the net does not use; 5x8 (smaller than a tile and than the halo), 8x32 (exactly one tile),
# 9x36 and 17x68 (partial tiles on both axes, 2 and 3 x 3 workgroups)
FUSED_SHAPES = ((8, (3, 5, 7)), (8, (1, 3)), (16, (3, 5)), (16, (1, 3)), (32, (1, 3)), (16, (3, 5, 7)))
FUSED_SIZES = ((5, 8), (8, 32), (9, 36), (17, 68))
FUSED_N = 3
FUSED_CASES = tuple((c, ks, H, W, aff) for c, ks in FUSED_SHAPES for H, W in FUSED_SIZES for aff in (False, True))

# channels-last kernels: sizes around the 32 x 8 tile
CL_SHAPES = ((8, (3, 5, 7)), (8, (1, 3)), (16, (3, 5)), (16, (1, 3)), (32, (1, 3)))        # = ops.DYNCONV_CL_SHAPES (asserted on the GPU)
CL_SIZES = ((1, 1), (3, 2), (5, 7), (8, 32), (9, 33), (17, 70))
CL_CASES = tuple((c, ks, H, W, N) for c, ks in CL_SHAPES for H, W in CL_SIZES for N in (1, 3))
CONV00_N = 3
CONV00_CASES = tuple((H, W, n_shared, bias) for H, W in CL_SIZES for n_shared in (1, 2, CONV00_N) for bias in (False, True))


def blend_case(K, c, H, W, N, n_shared):
    return make_blend_case(1000 + 97 * K + 13 * c + H * W + n_shared, K, c, N, n_shared, H, W, epi_start=(c + H) % 5)


def fused_case(c, ks, H, W, aff):
    return make_conv_case(2000 + 31 * c + 7 * sum(ks) + H * W, c, c, ks, FUSED_N, 1, H, W, aff, True, epi_start=(c + len(ks) + H) % 5)


def cl_case(c, ks, H, W, N):
    """Bias on every second case, always the pending affine (the split-f16 kernels are told a bound on the input AFTER it)."""
    i = CL_CASES.index((c, ks, H, W, N))
    return make_conv_case(3000 + 17 * c + 5 * sum(ks) + H * W + N, c, c, ks, N, 1, H, W, True, i % 2 == 0, epi_start=i % 5)


def conv00_case(H, W, n_shared, bias):
    S = CONV00_N - n_shared + 1
    return make_conv_case(4000 + H * W + 3 * n_shared + int(bias), 3, 8, (3, 7, 11), S, n_shared, H, W, False, bias, image=True,
                          epi_start=(H + n_shared) % 5)


def all_cases():
    """(family, id, case) of every case of section 3: what the CPU test measures the constants and the loose-pixel shares on."""
    for p in BLEND_CASES:
        yield "blend", p, blend_case(*p)
    for p in FUSED_CASES:
        yield "fused_sbf", p, fused_case(*p)
    for p in CL_CASES:
        yield "dynconv_cl", p, cl_case(*p)
    for p in CONV00_CASES:
        yield "conv00_cl", p, conv00_case(*p)
