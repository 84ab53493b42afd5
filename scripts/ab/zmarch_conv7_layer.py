"""conv7 (ConvTranspose3d 64 -> 32 + ReLU + residual, split-f16) on its own: tiled kernel (CDS_DZM_DEEP=0) against the z-march
(CDS_DZM_DEEP=2) in alternating pairs at the headline and cascade volumes, and the z-segment scan at M1.  HIP events around 20 launches
on the same tensors, so L2 / the memory-side cache are warm: lower than in the step.  Usage: zmarch_conv7_layer.py [pairs]"""
import os, sys, torch
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
from cds_mvsnet_amd import ops
dev = torch.device("cuda")
PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
# input cells of conv7: M1; stage 1 / 2 / 3 of the 1600x1184 cascade; stage 2 / 3 of the 640x512 cascade
SHAPES = {"M1": (24, 64, 80), "M3s1": (6, 37, 50), "M3s2": (4, 74, 100), "M3s3": (1, 148, 200), "M2s2": (4, 32, 40), "M2s3": (1, 64, 80)}


def t(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


g = torch.Generator().manual_seed(0)
w = torch.randn(64, 32, 3, 3, 3, generator=g) / (27 * 8) ** 0.5
wh, w_inv = ops.split_pack_deconv3d(w.to(dev), f16=True)
bias = torch.randn(32, generator=g).to(dev)
for name, (D, H, W) in SHAPES.items():
    x = torch.randn(D, H, W, 64, device=dev)
    skip = torch.randn(2 * D, 2 * H, 2 * W, 32, device=dev)
    bound = x.abs().amax().reshape(1)
    fn = lambda: ops.deconv3d_sbf(x, wh, bias, 32, skip=skip, in_bound=bound, w_inv_scale=w_inv)
    os.environ.pop("CDS_DZM_NSEG", None)
    res = {"0": [], "2": []}
    for _ in range(PAIRS):
        for deep in ("0", "2"):
            os.environ["CDS_DZM_DEEP"] = deep
            res[deep].append(t(fn))
    os.environ["CDS_DZM_DEEP"] = "1"
    auto = t(fn)
    print(f"{name} {D}x{H}x{W}: tiled " + " ".join(f"{v:.1f}" for v in res["0"]) + " | z-march " + " ".join(f"{v:.1f}" for v in res["2"])
          + f" | default knob {auto:.1f} us", flush=True)
    if name == "M1":
        os.environ["CDS_DZM_DEEP"] = "2"
        for nseg in (1, 2, 3, 4, 6, 8, 12):
            os.environ["CDS_DZM_NSEG"] = str(nseg)
            print(f"  M1 z segments {nseg}: {t(fn):.1f} {t(fn):.1f} us", flush=True)
        os.environ.pop("CDS_DZM_NSEG", None)
    del x, skip
