"""The visibility CNN on its own: the row-marching kernel (ops.vis_cnn_rm, csrc/vis_rm.hip) against the three launches it replaces,
20 launches each, at the M1 shape and at the three stage shapes of the 1600x1184 and 1920x1056 cascades (4 source views), and the
CDS_VIS_NSEG sweep at M1.  Usage: vis_rowmarch_layer.py [V]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from cds_mvsnet_amd import ops
from cds_mvsnet_amd.model import _pack2d

V = int(sys.argv[1]) if len(sys.argv) > 1 else 4
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
w0, b0 = torch.randn(16, 2, 3, 3, generator=g) / 4.0, torch.randn(16, generator=g) * 0.2
ws, bs = [], []
for _ in range(2):
    ws.append(ops.split_pack_dynconv([(torch.randn(16, 16, 3, 3, generator=g) / 12.0).to(dev)]))
    bs.append((torch.randn(16, generator=g) * 0.2).to(dev))
hw, hb = (torch.randn(16, generator=g) * 0.3).to(dev), torch.randn(1, generator=g).to(dev)
wp, b0 = _pack2d(w0.to(dev)), b0.to(dev)


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / n * 1e3          # us


def three(ent, nc):
    x = ops.vis_layer1_cl(ent, nc, wp, b0)
    x = ops.conv2d_k3_relu_cl(x, ws[0], bs[0])
    return ops.conv2d_k3_relu_cl(x, ws[1], bs[1], head_w=hw, head_b=hb)


def fused(ent, nc):
    return ops.vis_cnn_rm(ent, nc, wp, b0, ws[0], bs[0], ws[1], bs[1], hw, hb)


shapes = [("M1", 512, 640)]
for name, H, W in (("1600x1184", 1184, 1600), ("1920x1056", 1056, 1920)):
    shapes += [(f"{name} stage {s + 1}", H >> (2 - s), W >> (2 - s)) for s in range(3)]
shapes += [("160x128, 2 views", 128, 160)]
os.environ.pop("CDS_VIS_NSEG", None)
for name, H, W in shapes:
    v = 2 if "2 views" in name else V
    ent, nc = torch.rand(v, H, W, generator=g).to(dev) * 3.0, torch.rand(v, H, W, generator=g).to(dev)
    same = torch.equal(three(ent, nc), fused(ent, nc))
    t3 = [timeit(lambda: three(ent, nc)) for _ in range(2)]
    tf = [timeit(lambda: fused(ent, nc)) for _ in range(2)]
    print(f"{name:22s} V={v} {W}x{H}: three launches {min(t3):7.1f} us  fused {min(tf):7.1f} us  ratio {min(t3) / min(tf):.2f}  equal {same}", flush=True)
ent, nc = torch.rand(V, 512, 640, generator=g).to(dev) * 3.0, torch.rand(V, 512, 640, generator=g).to(dev)
for nseg in (1, 2, 4, 6, 8, 11, 13, 17, 22, 26, 32, 43, 64):
    os.environ["CDS_VIS_NSEG"] = str(nseg)
    print(f"M1 CDS_VIS_NSEG={nseg:3d}: fused {timeit(lambda: fused(ent, nc)):7.1f} us", flush=True)
os.environ.pop("CDS_VIS_NSEG", None)
print(f"M1 default segments: fused {timeit(lambda: fused(ent, nc)):7.1f} us")
