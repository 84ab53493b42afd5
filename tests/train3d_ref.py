"""Float64 references, error bars and case lists of the CostRegNet fp32 training kernels (csrc/train3d.hip, cds_pack_conv3d_f32):
CPU torch only, nothing of the library under test.  tests/test_train3d_ref_cpu.py checks this file against autograd and a float32
emulation of the kernels' formulas; tests/test_train3d_gpu.py compares the kernels with it and takes every case list from here."""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24            # unit roundoff of float32
EXACT_LIMIT = 2.0 ** 24   # every integer below it is a float32: sums of integer terms that stay below it are exact in any order

# ---- case lists (shared by the CPU and the GPU file) ----------------------------------------------------------------------------------
# every (Cin, Cout, stride, transposed) of CostRegNet(C, 8), C in {8, 16, 32} (tests/test_train_sf16_gpu.py LAYERS) and its prob layer
from test_train_sf16_gpu import LAYERS as _UNET_LAYERS  # noqa: E402

LAYER_CASES = list(_UNET_LAYERS) + [(8, 1, 1, False)]
LAYER_VOLUMES = [(6, 10, 40), (8, 8, 8)]
LAYER_BATCH = 2

# conv3d_wgrad: (B, Ca, Cb, g volume, xin volume, S); the kernels' tile is 8 x 4 x 4 voxels of g (x, y, z)
WGRAD_CASES = [
    (1, 16, 8, (1, 1, 1), (1, 1, 1), 1),          # only the centre tap may be non-zero
    (2, 8, 8, (5, 6, 11), (5, 6, 11), 1),         # tails on all three axes
    (2, 19, 11, (4, 5, 9), (4, 5, 9), 1),         # two a-blocks and two b-blocks, both partial
    (1, 1, 8, (6, 10, 20), (6, 10, 20), 1),       # the prob layer
    (2, 16, 8, (4, 5, 9), (7, 9, 17), 2),         # odd input: its last slice is read by tap 2 only
    (2, 16, 8, (4, 5, 8), (8, 10, 16), 2),        # even input
    (2, 64, 32, (1, 2, 3), (2, 4, 6), 2),         # transposed role (g = x, xin = dy): CostRegNet's deepest level
    (2, 32, 16, (3, 5, 9), (6, 10, 18), 2),       # transposed role
]
# 18 tiles per item, 54 in all: CDS_WG3_WGS unset -> 1 tile per workgroup; 5 -> 11 (workgroups start mid-item and cross both batch
# boundaries, the last one has 10); 1 -> one workgroup per channel block marches all 54
WGRAD_TILE_CASES = [(3, 16, 8, (6, 9, 20), (6, 9, 20), 1), (3, 16, 8, (6, 9, 20), (11, 18, 39), 2)]
WGRAD_TILE_WGS = [None, "5", "1"]

# BnRelu3d: (B, C, D, H, W)
BN_SHAPES = [
    (2, 16, 8, 12, 20),       # V = 1920: float4 path
    (2, 64, 1, 2, 3),         # V = 6: scalar path
    (1, 8, 3, 5, 7),          # V = 105: scalar path
    (3, 1, 4, 36, 36),        # V = 5184, three chunks: some threads of the statistics pass take the paired iteration, others the tail
]
BN_CHUNKED_SHAPE, BN_CHUNKS = (2, 16, 8, 12, 20), ["1", "3"]       # CDS_BN_RED_CHUNKS: many iterations of both reductions
BN_BIG_SHAPES = [(1, 2, 9, 256, 512), (1, 2, 9, 257, 511)]         # V > 512 * 2048: the normalisation passes loop twice (float4, scalar)
BN_ALIGN_SHAPE = (2, 8, 2, 4, 8)                                   # V % 4 == 0
BN_OFFSETS = [0.0, 1.0, 30.0]                                      # channel mean in units of the channel's sigma
BN_MOMENTA = [0.1, 1.0, None]                                      # None: no running statistics
BN_EPS = 1e-5


def all_bn_shapes():
    return BN_SHAPES + [BN_CHUNKED_SHAPE] + BN_BIG_SHAPES + [BN_ALIGN_SHAPE]


# ---- convolutions ---------------------------------------------------------------------------------------------------------------------
def wgrad_ref(g, xin, stride):
    """dw[a][b][kz][ky][kx] = sum over batch and o of g[a][o] * xin[b][S o - 1 + k] (zero outside xin), float64: the header of
    csrc/train3d.hip written out, one zero-padded shifted strided slice and one contraction per tap."""
    g, xin = g.double(), xin.double()
    B, Ca, Do, Ho, Wo = g.shape
    S = stride
    # padded index S o + k, k in 0..2: lengths S (n_o - 1) + 3
    hi = [max(0, S * (no - 1) + 2 - ni) for no, ni in zip((Do, Ho, Wo), xin.shape[2:])]
    xp = F.pad(xin, (1, hi[2], 1, hi[1], 1, hi[0]))
    dw = torch.zeros(Ca, xin.shape[1], 3, 3, 3, dtype=torch.float64)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                sl = xp[:, :, kz:kz + S * (Do - 1) + 1:S, ky:ky + S * (Ho - 1) + 1:S, kx:kx + S * (Wo - 1) + 1:S]
                dw[:, :, kz, ky, kx] = torch.einsum("nadhw,nbdhw->ab", g, sl)
    return dw


def conv_ref(x, w, stride, transposed):
    return F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1) if transposed else F.conv3d(x, w, stride=stride, padding=1)


def layer_ref(x, w, gout, stride, transposed, dtype):
    """(y, dx, dw) of one k3 layer in `dtype` through PyTorch's convolution and autograd."""
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    wr = w.detach().to(dtype).clone().requires_grad_(True)
    y = conv_ref(xr, wr, stride, transposed)
    y.backward(gout.to(dtype))
    return y.detach(), xr.grad, wr.grad


def layer_shapes(cin, cout, stride, transposed, vol, B=LAYER_BATCH):
    """(x shape, w shape, y shape); for a transposed layer the volume is its output, as in CostRegNet."""
    D, H, W = (v // 2 for v in vol) if transposed else vol
    xs = (B, cin, D, H, W)
    ws = ((cin, cout) if transposed else (cout, cin)) + (3, 3, 3)
    if transposed:
        ys = (B, cout, 2 * D, 2 * H, 2 * W)
    else:
        ys = (B, cout) + tuple((d - 1) // stride + 1 for d in (D, H, W))
    return xs, ws, ys


def _ints(shape, lim, gen):
    return torch.randint(-lim, lim + 1, shape, generator=gen).float()


def _scaled(shape, gen):
    """randn with uneven per-channel scales (dimension 1)."""
    sc = [1] * len(shape)
    sc[1] = shape[1]
    return torch.randn(shape, generator=gen) * torch.exp(torch.randn(sc, generator=gen))


def _seed(*key):
    return int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) % (2 ** 31)


def int_case(kind, *key):
    """Small integers stored as float32: activations and gradients in -3..3, weights in -2..2.  Every product and every partial sum
    is then an exact float32 (on the VALU, the fp32 MFMA and in the split forward alike) as long as sum |terms| < 2^24 per output
    element (exact_headroom), so a kernel must reproduce the float64 reference bit for bit whatever its summation or atomic order.
    kind "wgrad": key = a WGRAD case -> (g, xin); kind "layer": key = (cin, cout, stride, transposed, vol) -> (x, w, gout)."""
    if kind == "wgrad":
        B, Ca, Cb, gv, xv, S = key
        gen = torch.Generator().manual_seed(_seed(B, Ca, Cb, *gv, *xv, S))
        return _ints((B, Ca) + tuple(gv), 3, gen), _ints((B, Cb) + tuple(xv), 3, gen)
    cin, cout, stride, transposed, vol = key
    gen = torch.Generator().manual_seed(_seed(cin, cout, stride, transposed, *vol))
    xs, ws, ys = layer_shapes(cin, cout, stride, transposed, vol)
    return _ints(xs, 3, gen), _ints(ws, 2, gen), _ints(ys, 3, gen)


def real_case(kind, *key):
    """The same shapes with real values: uneven per-channel scales; weights ~ 1 / sqrt(fan-in), output gradients ~ 1e-3."""
    if kind == "wgrad":
        B, Ca, Cb, gv, xv, S = key
        gen = torch.Generator().manual_seed(_seed(B, Ca, Cb, *gv, *xv, S) + 1)
        return _scaled((B, Ca) + tuple(gv), gen) * 1e-3, _scaled((B, Cb) + tuple(xv), gen)
    cin, cout, stride, transposed, vol = key
    gen = torch.Generator().manual_seed(_seed(cin, cout, stride, transposed, *vol) + 1)
    xs, ws, ys = layer_shapes(cin, cout, stride, transposed, vol)
    return _scaled(xs, gen), torch.randn(ws, generator=gen) / (27 * cin) ** 0.5, torch.randn(ys, generator=gen) * 1e-3


def exact_headroom(kind, case, stride, transposed=False):
    """max over output elements of sum |terms| for the integer case: must be < EXACT_LIMIT."""
    if kind == "wgrad":
        g, xin = case
        return wgrad_ref(g.abs(), xin.abs(), stride).max().item()
    x, w, gout = case
    return max(t.max().item() for t in layer_ref(x.abs(), w.abs(), gout.abs(), stride, transposed, torch.float64))


def wgrad_torch(g, xin, stride, dtype):
    """PyTorch's own weight gradient of conv3d(xin, w, stride, padding 1) for the output gradient g, in `dtype`."""
    w = torch.zeros(g.shape[1], xin.shape[1], 3, 3, 3, dtype=dtype, requires_grad=True)
    y = F.conv3d(xin.to(dtype), w, stride=stride, padding=1)
    assert y.shape == g.shape, (y.shape, g.shape)
    y.backward(g.to(dtype))
    return w.grad


def fp32_class_bar(r64, r32, margin=4.0):
    """(err32, bar): the bar of a real-valued result, margin x PyTorch's own fp32 error of the same pass + one ulp of the result scale.
    It only has to separate fp32-class arithmetic from the next class down (a dropped low-order split term, single bf16: >= 2^8
    worse); the margin of 4 covers a different summation order (the kernels sum 128-voxel tiles serially per lane, then use atomics)
    and was chosen before any measurement."""
    err32 = (r32.double() - r64).abs().max().item()
    return err32, margin * err32 + r64.abs().max().item() * 2.0 ** -23


# ---- BatchNorm + ReLU + skip -----------------------------------------------------------------------------------------------------------
def bn_ref(y, gamma, beta, skip, dout, running, momentum, eps, relu):
    """out = [skip +] relu?(batch_norm_train(y)) in float64 with autograd.  running: (mean, var) or None (not modified).
    -> dict(out, dy, dgamma, dbeta, dskip, running_mean, running_var, pre)."""
    yr = y.double().clone().requires_grad_(True)
    gr = gamma.double().clone().requires_grad_(True)
    br = beta.double().clone().requires_grad_(True)
    sr = skip.double().clone().requires_grad_(True) if skip is not None else None
    rm, rv = (running[0].double().clone(), running[1].double().clone()) if running is not None else (None, None)
    pre = F.batch_norm(yr, rm, rv, gr, br, True, momentum if running is not None else 0.0, eps)
    out = torch.relu(pre) if relu else pre
    if sr is not None:
        out = sr + out
    out.backward(dout.double())
    return dict(out=out.detach(), dy=yr.grad, dgamma=gr.grad, dbeta=br.grad, dskip=sr.grad if sr is not None else None,
                running_mean=rm, running_var=rv, pre=pre.detach())


def bn_closed_form(y, gamma, beta, dout, eps, relu):
    """The per-channel quantities of the kernels' closed forms in float64 (comments of bn3d_norm_kernel / bn3d_bwd_norm_kernel):
    sc = gamma invstd, sh = beta - mean sc, pre = y sc + sh, g = dout [pre > 0], db = sum g, dg = sum g xhat,
    a1 = -sc dg invstd / n, a0 = -sc db / n + sc dg invstd mean / n, dy = g sc + y a1 + a0."""
    y, dout = y.double(), dout.double()
    C = y.shape[1]
    v = (1, C, 1, 1, 1)
    n = y.numel() // C
    mean = y.mean((0, 2, 3, 4))
    var = ((y - mean.view(v)) ** 2).mean((0, 2, 3, 4))
    invstd = 1.0 / torch.sqrt(var + eps)
    sc = gamma.double() * invstd
    sh = beta.double() - mean * sc
    pre = y * sc.view(v) + sh.view(v)
    g = dout * (pre > 0) if relu else dout
    xhat = (y - mean.view(v)) * invstd.view(v)
    db = g.sum((0, 2, 3, 4))
    dg = (g * xhat).sum((0, 2, 3, 4))
    a1 = -sc * dg * invstd / n
    a0 = -sc * db / n + sc * dg * invstd * mean / n
    dy = g * sc.view(v) + y * a1.view(v) + a0.view(v)
    return dict(n=n, mean=mean, var=var, invstd=invstd, sc=sc, sh=sh, pre=pre, g=g, xhat=xhat, db=db, dg=dg, a1=a1, a0=a0, dy=dy)


def pre_bar(q, y):
    """Rounding bound of the kernels' pre-activation fmaf(y, sc, sh): one float rounding each of sc, sh and of the fmaf; margin 2."""
    v = (1, -1, 1, 1, 1)
    return 2 * U * ((y.double() * q["sc"].view(v)).abs() + q["sh"].abs().view(v) + q["pre"].abs())


def bn_bars(y, gamma, beta, skip, dout, running, momentum, eps, relu):
    """The rounding model of the kernels' closed forms, from float64 reference quantities only (u = 2^-24, margin 2).
    forward   2u (|y sc| + |sh| + |pre|), + 2u |out| when a skip is added
    backward  2u (|g sc| + 2 |y a1| + 2 |a0| + |dy|)
      one float rounding each of sc, sh, a1, a0, one per fmaf; a1 and a0 are built from the rounded sc
    dgamma 2^-22 sum |g xhat|, dbeta 2^-22 sum |g|, running statistics 4u (|r| + |stat|); dskip is dout itself (bar 0)."""
    q = bn_closed_form(y, gamma, beta, dout, eps, relu)
    v = (1, -1, 1, 1, 1)
    yd = y.double()
    out_bar = pre_bar(q, y)
    if skip is not None:
        out = skip.double() + (torch.relu(q["pre"]) if relu else q["pre"])
        out_bar = out_bar + 2 * U * out.abs()
    dy_bar = 2 * U * ((q["g"] * q["sc"].view(v)).abs() + 2 * (yd * q["a1"].view(v)).abs() + 2 * q["a0"].abs().view(v) + q["dy"].abs())
    bars = dict(out=out_bar, dy=dy_bar, dgamma=2.0 ** -22 * (q["g"] * q["xhat"]).abs().sum((0, 2, 3, 4)),
                dbeta=2.0 ** -22 * q["g"].abs().sum((0, 2, 3, 4)))
    if running is not None:
        n = q["n"]
        unbiased = q["var"] * (n / (n - 1.0 if n > 1 else 1.0))
        bars["running_mean"] = 4 * U * (running[0].double().abs() + q["mean"].abs())
        bars["running_var"] = 4 * U * (running[1].double().abs() + unbiased.abs())
    return bars


def relu_boundary_violations(y, gamma, beta, eps=BN_EPS):
    """How many pre-activations lie closer to 0 than their forward bar.  A ReLU mask bit the kernel could round the other way changes
    sum g and with it every dy of its channel, so the GPU tests exclude nothing and use inputs for which this is 0."""
    q = bn_closed_form(y, gamma, beta, torch.zeros_like(y), eps, True)
    return int((q["pre"].abs() < pre_bar(q, y)).sum())


@functools.lru_cache(maxsize=4)
def bn_case(shape, offset):
    """dict(y, gamma, beta, skip, dout, running_mean, running_var, offset): y = sigma_c (randn + offset) with uneven sigma_c.  Pre-activations
    the float64 reference puts within their bar of the ReLU boundary are moved away from it by sigma_c / 256 (a few elements per
    million at offset 30), until relu_boundary_violations is 0.  The tensors are shared between tests: do not modify them."""
    B, C, D, H, W = shape
    gen = torch.Generator().manual_seed(_seed(B, C, D, H, W, int(offset)))
    sigma = torch.exp(0.5 * torch.randn(1, C, 1, 1, 1, generator=gen))
    y = sigma * (torch.randn(shape, generator=gen) + offset)
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen)
    skip = torch.randn(shape, generator=gen)
    dout = torch.randn(shape, generator=gen)
    rmean = torch.randn(C, generator=gen)
    rvar = torch.rand(C, generator=gen) + 0.5
    for _ in range(8):
        q = bn_closed_form(y, gamma, beta, dout, BN_EPS, True)
        near = q["pre"].abs() < 4 * pre_bar(q, y)
        if not near.any():
            break
        push = torch.where(q["pre"] >= 0, 1.0, -1.0) * torch.sign(q["sc"]).view(1, C, 1, 1, 1) * (sigma.double() / 256)
        y = torch.where(near, (y.double() + push).float(), y)
    return dict(y=y, gamma=gamma, beta=beta, skip=skip, dout=dout, running_mean=rmean, running_var=rvar, offset=offset)


def bn_emulate_f32(y, gamma, beta, skip, dout, running, momentum, eps, relu):
    """The kernels' formulas step by step with their roundings: float64 statistics and per-channel steps, sc / sh / a1 / a0 rounded to
    float32, one rounding per fmaf (a float32 product is exact in float64), float32 running-statistics update."""
    def fma(a, b, c):
        return (a.double() * b.double() + c.double()).float()

    C = y.shape[1]
    v = (1, C, 1, 1, 1)
    n = float(y.numel() // C)
    yd = y.double()
    s, q = yd.sum((0, 2, 3, 4)), (yd * yd).sum((0, 2, 3, 4))
    mean = s / n
    var = (q / n - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    gm = gamma.double()
    sc = (gm * invstd).float()
    sh = (beta.double() - mean * gm * invstd).float()
    res = {}
    if running is not None:
        m = torch.tensor(momentum, dtype=torch.float32)
        one = torch.tensor(1.0, dtype=torch.float32)
        res["running_mean"] = running[0] * (one - m) + m * mean.float()
        res["running_var"] = running[1] * (one - m) + m * (var * (n / (n - 1.0 if n > 1 else 1.0))).float()
    pre = fma(y, sc.view(v).expand_as(y), sh.view(v).expand_as(y))
    out = torch.relu(pre) if relu else pre
    res["out"] = skip + out if skip is not None else out
    g = torch.where(pre > 0, dout, torch.zeros_like(dout)) if relu else dout
    gs, gy = g.double().sum((0, 2, 3, 4)), (g.double() * yd).sum((0, 2, 3, 4))
    dg = invstd * (gy - mean * gs)
    scd = sc.double()
    a1 = (-scd * dg * invstd / n).float()
    a0 = (-scd * gs / n + scd * dg * invstd * mean / n).float()
    res["dy"] = fma(g, sc.view(v).expand_as(y), fma(y, a1.view(v).expand_as(y), a0.view(v).expand_as(y)))
    res["dgamma"], res["dbeta"] = dg.float(), gs.float()
    res["dskip"] = dout if skip is not None else None
    return res


def bn_compare(got, ref, bars):
    """[(name, max err, max bar, number of elements with err > bar)] over everything a BnRelu3d call produces; dskip must be dout
    itself.  err <= bar element by element, never a ratio: a bar is 0 where every term is (a channel the ReLU switches off)."""
    rows = []
    for name in ("out", "dy", "dgamma", "dbeta", "running_mean", "running_var"):
        if name not in bars:
            continue
        err = (got[name].double() - ref[name]).abs()
        bad = int((~(err <= bars[name])).sum())          # a nan counts as a miss
        rows.append((name, err.max().item(), bars[name].max().item(), bad))
    if ref["dskip"] is not None:
        rows.append(("dskip", (got["dskip"].double() - ref["dskip"]).abs().max().item(), 0.0, int((got["dskip"].double() != ref["dskip"]).sum())))
    return rows
