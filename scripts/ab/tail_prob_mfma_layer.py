"""The fused CostRegNet tail (conv11 + conv0 residual + prob, split-f16) on its own: prob on the VALU (CDS_DPZ_PROB_MFMA=0, the kernel
of the parent commit) against prob on the matrix cores, alternating in one process at the headline and cascade stage volumes.  HIP
events around 20 launches on the same tensors.  Usage: tail_prob_mfma_layer.py [pairs]"""
import os, sys, torch
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
from cds_mvsnet_amd import ops
dev = torch.device("cuda")
PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
# input cells of conv11: M1; stages 1 / 2 / 3 of the 1600x1184 and 1920x1056 cascades; stage 3 of the 640x512 cascade
SHAPES = {"M1": (96, 256, 320), "M3s1": (24, 148, 200), "M3s2": (16, 296, 400), "M3s3": (4, 592, 800),
          "M4s1": (24, 132, 240), "M4s2": (16, 264, 480), "M4s3": (4, 528, 960), "M2s3": (4, 256, 320)}


def t(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


g = torch.Generator().manual_seed(0)
w11 = torch.randn(16, 8, 3, 3, 3, generator=g) / (27 * 2) ** 0.5
wp = torch.randn(1, 8, 3, 3, 3, generator=g) / 27 ** 0.5
wh, w_inv = ops.split_pack_deconv_prob(w11.to(dev), f16=True)
wm, wm_inv = ops.split_pack_prob(wp.to(dev), f16=True)
tab = ops.pack_prob_table(wp.to(dev))
bias = torch.randn(8, generator=g).to(dev)
gain = ops.deconv_prob_gain(wh, w_inv)
for name, (D, H, W) in SHAPES.items():
    x = torch.randn(D, H, W, 16, device=dev)
    skip = torch.randn(2 * D, 2 * H, 2 * W, 8, device=dev)
    bound, sb = x.abs().amax().reshape(1), skip.abs().amax().reshape(1)
    fn = lambda: ops.deconv_prob_zm(x, wh, bias, skip, tab, in_bound=bound, w_inv_scale=w_inv, prob_mfma=wm, prob_inv_scale=wm_inv,
                                    skip_bound=sb, y_gain=gain)
    res = {"0": [], "1": []}
    for _ in range(PAIRS):
        for k in ("0", "1"):
            os.environ["CDS_DPZ_PROB_MFMA"] = k
            res[k].append(t(fn))
    print(f"{name} {D}x{H}x{W}: VALU " + " ".join(f"{v:.1f}" for v in res["0"]) + " | matrix cores " + " ".join(f"{v:.1f}" for v in res["1"])
          + " us", flush=True)
    del x, skip
