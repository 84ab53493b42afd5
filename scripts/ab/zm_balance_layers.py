"""Every z-march layer of CostRegNet on its own, uniform cutting (CDS_ZM_BALANCE=0) against the balanced one (=2, forced) in alternating
pairs, and what the default (=1) runs, at the M1 volume and the stage volumes of the 640x512, 1600x1184 and 1920x1056 cascades.  HIP
events around N launches on the same tensors (caches warm: lower than in the step).  profiles/zm_balance.md holds the results.
Usage: zm_balance_layers.py [pairs] [volume names ...]"""
import ctypes, os, sys, torch
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
from cds_mvsnet_amd import _lib, ops
dev = torch.device("cuda")
PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
# full-resolution volume of a stage's CostRegNet (D, H, W) and the channels of its input
VOLS = {"M1": ((192, 512, 640), 8),
        "M2s1": ((48, 128, 160), 32), "M2s2": ((32, 256, 320), 16), "M2s3": ((8, 512, 640), 8),
        "M3s1": ((48, 296, 400), 32), "M3s2": ((32, 592, 800), 16), "M3s3": ((8, 1184, 1600), 8),
        "M4s1": ((48, 264, 480), 32), "M4s2": ((32, 528, 960), 16), "M4s3": ((8, 1056, 1920), 8)}
names = sys.argv[2:] or list(VOLS)
lib = _lib.load()


def t(fn, n=10):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def half(v, k=1):
    for _ in range(k): v = tuple((x - 1) // 2 + 1 for x in v)
    return v


def plan(fam, cols, planes, unit, ys):
    o = (ctypes.c_int * 4)()
    lib.cds_zm_plan(fam, cols, planes, unit, ys, 256, 1, o)
    return f"model {o[2] / 1000:.1f} -> {o[3] / 1000:.1f}, default {'balanced' if o[0] else 'uniform'}"


def cd(a, b): return -(-a // b)


g = torch.Generator().manual_seed(0)
for vn in names:
    V, c0 = VOLS[vn]
    layers = []

    def conv(name, cin, cout, stride, vin, tile, pair=False):
        w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
        wh, w_inv = (ops.split_pack_conv3d_pair if pair else ops.split_pack_conv3d)(w.to(dev), f16=True)
        bias = torch.randn(cout, generator=g).to(dev)
        x = torch.randn(*vin, cin, device=dev)
        bound = x.abs().amax().reshape(1)
        fn = lambda: ops.conv3d_sbf(x, wh, bias, cout, stride=ops.SBF_PAIR if pair else stride, relu=True, in_bound=bound, w_inv_scale=w_inv)
        vo = half(vin) if stride == 2 else vin
        txo, tyo, G, ys = tile
        layers.append((name, fn, plan(0, cd(vo[2], txo) * cd(vo[1], tyo), vo[0], G, ys)))

    def deconv(name, cin, cout, vin):
        w = torch.randn(cin, cout, 3, 3, 3, generator=g) / (27 * cin / 8) ** 0.5
        x = torch.randn(*vin, cin, device=dev)
        skip = torch.randn(*(2 * v for v in vin), cout, device=dev)
        bias = torch.randn(cout, generator=g).to(dev)
        bound = x.abs().amax().reshape(1)
        if cout == 32:
            wh, w_inv = ops.split_pack_deconv3d(w.to(dev), f16=True)
            fn = lambda: ops.deconv3d_sbf(x, wh, bias, 32, relu=True, skip=skip, in_bound=bound, w_inv_scale=w_inv)
            layers.append((name, fn, plan(1, cd(vin[2], 16) * cd(vin[1], 4), vin[0], 1, 2)))
        else:
            wh, w_inv = ops.split_pack_deconv_cls(w.to(dev), f16=True)
            fn = lambda: ops.deconv3d_zm(x, wh, bias, relu=True, skip=skip, in_bound=bound, w_inv_scale=w_inv)
            layers.append((name, fn, plan(1, cd(vin[2], 16) * cd(vin[1], 8), vin[0], 1, 1)))

    def tail(vin):
        x = torch.randn(*vin, 16, device=dev)
        skip = torch.randn(*(2 * v for v in vin), 8, device=dev)
        w11 = torch.randn(16, 8, 3, 3, 3, generator=g).to(dev) / (27 * 2) ** 0.5
        wp = torch.randn(1, 8, 3, 3, 3, generator=g).to(dev) / 27 ** 0.5
        wh, w_inv = ops.split_pack_deconv_prob(w11, f16=True)
        wm, wms = ops.split_pack_prob(wp, f16=True)
        b, tab = torch.randn(8, generator=g).to(dev), ops.pack_prob_table(wp)
        ib, sb, gain = x.abs().amax().reshape(1), skip.abs().amax().reshape(1), ops.deconv_prob_gain(wh, w_inv)
        fn = lambda: ops.deconv_prob_zm(x, wh, b, skip, tab, in_bound=ib, w_inv_scale=w_inv, prob_mfma=wm, prob_inv_scale=wms, skip_bound=sb, y_gain=gain)
        layers.append(("tail", fn, plan(2, cd(vin[2], 30) * cd(vin[1], 6), vin[0], 1, 1)))

    # one layer at a time: build, time, free
    specs = [lambda: conv("conv0", c0, 8, 1, V, {8: (32, 8, 3, 1), 16: (32, 8, 1, 1), 32: (32, 3, 1, 1)}[c0], pair=True),
             lambda: conv("conv1", 8, 16, 2, V, (16, 8, 1, 1)), lambda: conv("conv2", 16, 16, 1, half(V), (32, 8, 1, 1)),
             lambda: conv("conv3", 16, 32, 2, half(V), (16, 4, 1, 1)), lambda: conv("conv4", 32, 32, 1, half(V, 2), (16, 4, 1, 1)),
             lambda: conv("conv5", 32, 64, 2, half(V, 2), (16, 2, 1, 1)), lambda: conv("conv6", 64, 64, 1, half(V, 3), (16, 2, 1, 2)),
             lambda: deconv("conv7", 64, 32, half(V, 3)), lambda: deconv("conv9", 32, 16, half(V, 2)), lambda: tail(half(V))]
    for spec in specs:
        layers.clear()
        spec()
        name, fn, pl = layers[0]
        res = {"0": [], "2": []}
        for _ in range(PAIRS):
            for bal in ("0", "2"):
                os.environ["CDS_ZM_BALANCE"] = bal
                res[bal].append(t(fn))
        os.environ["CDS_ZM_BALANCE"] = "1"
        auto = t(fn)
        wins = all(b < u for u, b in zip(res["0"], res["2"]))
        print(f"{vn} {name}: uniform " + " ".join(f"{v:.1f}" for v in res["0"]) + " | balanced " + " ".join(f"{v:.1f}" for v in res["2"])
              + f" | default {auto:.1f} us | {pl} | balanced lower in every pair: {wins}", flush=True)
        layers.clear()
        del fn
        torch.cuda.empty_cache()
