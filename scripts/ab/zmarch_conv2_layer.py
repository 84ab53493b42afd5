"""conv2 (Conv3d 16 -> 16 + ReLU, split-f16) on its own at the headline and cascade volumes, with the library CDS_MVSNET_LIB names (the
form of the layer is a property of the build: run this once per library, alternating, to compare two builds).  HIP events around 20
launches on the same tensors, so L2 / the memory-side cache are warm.  Prints one line: us per launch and a checksum of the output bits
per volume.  Usage: [CDS_MVSNET_LIB=other.so] zmarch_conv2_layer.py"""
import os, sys, torch
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
from cds_mvsnet_amd import ops
dev = torch.device("cuda")
# input voxels of conv2: M1; stage 1 / 2 / 3 of the 1600x1184 and of the 1920x1056 cascade
SHAPES = {"M1": (96, 256, 320), "M3s1": (24, 148, 200), "M3s2": (16, 296, 400), "M3s3": (4, 592, 800),
          "M4s1": (24, 132, 240), "M4s2": (16, 264, 480), "M4s3": (4, 528, 960)}


def t(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


g = torch.Generator().manual_seed(0)
w = torch.randn(16, 16, 3, 3, 3, generator=g) / (27 * 16) ** 0.5
wh, w_inv = ops.split_pack_conv3d(w.to(dev), f16=True)
bias = torch.randn(16, generator=g).to(dev)
res = []
for name, (D, H, W) in SHAPES.items():
    x = torch.randn(D, H, W, 16, generator=g).to(dev)
    bound = x.abs().amax().reshape(1)
    fn = lambda: ops.conv3d_sbf(x, wh, bias, 16, stride=1, relu=True, in_bound=bound, w_inv_scale=w_inv)
    chk = int(fn().view(torch.int32).to(torch.int64).sum())
    res.append(f"{name} {t(fn):.1f} ({chk % 1000000:06d})")
    del x
print(" | ".join(res), flush=True)
