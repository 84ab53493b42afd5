"""conv5 (Conv3d 32 -> 64 stride 2 + ReLU, split-f16) on its own: tiled kernel (CDS_ZMG_DEEP=0) against the z-march on the 32-byte ring
(CDS_ZMG_DEEP=2) in alternating pairs at the headline and cascade volumes, and the z-segment scan at M1.  HIP events around 20 launches
on the same tensors, so L2 / the memory-side cache are warm: lower than in the step.  Usage: zmarch_conv5_layer.py [pairs]"""
import os, sys, torch
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
from cds_mvsnet_amd import ops
dev = torch.device("cuda")
PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
# input voxels of conv5: M1; stage 1 / 2 / 3 of the 1600x1184 and of the 1920x1056 cascade; stage 1 of the 640x512 cascade
SHAPES = {"M1": (48, 128, 160), "M3s1": (12, 74, 100), "M3s2": (8, 148, 200), "M3s3": (2, 296, 400),
          "M4s1": (12, 66, 120), "M4s2": (8, 132, 240), "M4s3": (2, 264, 480), "M2s1": (12, 32, 40)}


def t(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


g = torch.Generator().manual_seed(0)
w = torch.randn(64, 32, 3, 3, 3, generator=g) / (27 * 32) ** 0.5
wh, w_inv = ops.split_pack_conv3d(w.to(dev), f16=True)
bias = torch.randn(64, generator=g).to(dev)
for name, (D, H, W) in SHAPES.items():
    x = torch.randn(D, H, W, 32, device=dev)
    bound = x.abs().amax().reshape(1)
    fn = lambda: ops.conv3d_sbf(x, wh, bias, 64, stride=2, relu=True, in_bound=bound, w_inv_scale=w_inv)
    os.environ.pop("CDS_ZMG_NSEG", None)
    res = {"0": [], "2": []}
    for _ in range(PAIRS):
        for deep in ("0", "2"):
            os.environ["CDS_ZMG_DEEP"] = deep
            res[deep].append(t(fn))
    os.environ["CDS_ZMG_DEEP"] = "1"
    auto = t(fn)
    print(f"{name} {D}x{H}x{W}: tiled " + " ".join(f"{v:.1f}" for v in res["0"]) + " | z-march " + " ".join(f"{v:.1f}" for v in res["2"])
          + f" | default knob {auto:.1f} us", flush=True)
    if name == "M1":
        os.environ["CDS_ZMG_DEEP"] = "2"
        for nseg in (1, 2, 3, 4, 6, 8):
            os.environ["CDS_ZMG_NSEG"] = str(nseg)
            print(f"  M1 z segments {nseg}: {t(fn):.1f} {t(fn):.1f} us", flush=True)
        os.environ.pop("CDS_ZMG_NSEG", None)
    del x
