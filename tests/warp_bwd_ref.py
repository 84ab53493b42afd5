"""Reference, inputs and a path model of the warp-aggregate (K3) backward, csrc/warp_bwd.hip: CPU torch only, nothing of the library
under test.  tests/test_warp_bwd_ref_cpu.py checks this file (against autograd through F.grid_sample) and the preconditions of the
cases; tests/test_warp_bwd_gpu.py compares the kernels with it.

  forward:  volume[c][d][p] = sum_v vis_v[p] * ref_v[c][p] * warp_v[c][d][p],   warp = zero-padded bilinear sample of src_v
  reference(): the gradients of sum(volume * G) w.r.t. ref / src / vis by autograd, in float64 (the reference) or float32 ("PyTorch's
  own fp32 error" of the same pass, the unit of the tests' bar).

The sample positions are the CPU oracle's (oracle.cds_oracle.sample_positions: the fp32 operation order of the model this project
follows, which the kernel recomputes; ops.WarpAggregate runs its forward with exact=True); they carry no gradient.  Everything after
them - the bilinear weights, the gather, the products and sums - is done here in the requested dtype.

box_plan() models which workgroups of the default kernel privatise their scatter in an LDS box, which fall back to direct global
atomics (box over CDS_K3BWD_BOX texels) and which are empty.  It is only ever a PRECONDITION on the inputs, with margins.
"""
import functools
import os
import re

import torch

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cds_mvsnet_amd", "csrc")

LEGACY_SHAPES = [(2, 8, 6, 12, 40), (3, 16, 4, 9, 70), (1, 32, 3, 8, 20), (2, 8, 40, 24, 130), (4, 16, 20, 33, 65)]   # test_warp_aggregate_backward_vs_autograd
ZERO_SHAPE = (2, 8, 40, 24, 130)        # the zero-branch and non-finite cases

# name -> (V, C, D, h, w): every parity case of tests/test_warp_bwd_gpu.py
CASES = {"legacy-%dx%dx%dx%dx%d" % s: s for s in LEGACY_SHAPES}
CASES.update({
    "seg-9+8": (2, 8, 17, 10, 70),          # two depth segments of 9 + 8 planes
    "seg-9+9+9+6": (2, 8, 33, 9, 66),       # four segments, the last one short; a 2-pixel tile remainder along x
    "seg-1": (1, 8, 15, 8, 20),             # one segment
    "shared-hyp": (2, 8, 24, 20, 70),       # hypotheses [D], the same for every pixel
    "nine-views": (9, 8, 4, 8, 20),         # more than MAX_VIEWS = 8: two launches
    "W-8": (3, 8, 40, 40, 130), "W-16": (3, 16, 40, 40, 130), "W-32": (3, 32, 40, 40, 130),
})


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _pack(feats, cams, hyp, seed):
    V = len(feats)
    _, C, h, w = feats[0]["ref"][0].shape
    D = hyp.shape[1]
    g = torch.Generator().manual_seed(seed)
    return dict(ref=torch.stack([f["ref"][0][0] for f in feats]), src=torch.stack([f["src"][0][0] for f in feats]), cams=cams, hyp=hyp,
                vis=torch.rand(V, h, w, generator=g) * 0.8 + 0.1, G=torch.randn(C, D, h, w, generator=g))


def stage_input(V, C, D, h, w):
    """The input family of the legacy test (tests/test_hip_parity.py _random_stage with seed 60 + V): friendly geometry."""
    from cds_mvsnet_amd import synth
    seed = 60 + V
    return _pack(synth.make_pair_features(V, C, h, w, seed=seed, sharp=True), synth.stage_cameras(V + 1, h, w, seed=seed + 1),
                 synth.make_hypotheses(D, h, w, seed=seed + 2), 5)


@functools.lru_cache(maxsize=None)
def case_input(name):
    """dict(ref [V,C,h,w], src [V,C,h,w], cams [1,V+1,2,4,4], hyp [1,D,h,w] or [1,D], vis [V,h,w], G [C,D,h,w]), float32, CPU.
    Cached: callers must not modify it."""
    from cds_mvsnet_amd import synth
    V, C, D, h, w = CASES[name]
    if name.startswith("W-"):
        import k3_chunk_plan as plan
        cams, hyp = plan.named_input("W", D)
        return _pack(plan.w_features(C), cams, hyp, 5)
    if name == "shared-hyp":
        return _pack(synth.make_pair_features(V, C, h, w, seed=10, sharp=True), synth.stage_cameras(V + 1, h, w, seed=11),
                     torch.linspace(425., 900., D).view(1, D), 5)
    return stage_input(V, C, D, h, w)


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def positions(cams, hyp, V, h, w):
    """[(ix, iy)] over the source views, each [D, h*w] float32: the oracle's sample positions (pixels)."""
    from oracle import cds_oracle as O
    P_ref = O.compose_projection(cams[:, 0])
    out = []
    for v in range(V):
        ix, iy = O.sample_positions(O.relative_projection(O.compose_projection(cams[:, v + 1]), P_ref), hyp, h, w)
        out.append((ix[0], iy[0]))
    return out


def taps(ix, iy, h, w):
    """The four taps (nw, ne, sw, se) of positions ix, iy (any float dtype): [(x, y, weight, inside)], x / y as floats."""
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx, ny = ix - x0, iy - y0
    ex, sy = 1 - wx, 1 - ny
    out = []
    for xi, yi, wt in ((x0, y0, sy * ex), (x0 + 1, y0, sy * wx), (x0, y0 + 1, ny * ex), (x0 + 1, y0 + 1, ny * wx)):
        out.append((xi, yi, wt, (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)))
    return out


def bilinear(src, ix, iy):
    """Zero-padded bilinear sample of src [C, h, w] at pixel positions ix, iy [D, hw] (align_corners=True un-normalised), in src's dtype:
    a tap outside the image contributes zero and receives no gradient.  -> [C, D, hw]"""
    C, h, w = src.shape
    flat = src.reshape(C, h * w)
    out = 0.0
    for xi, yi, wt, ok in taps(ix, iy, h, w):
        lin = torch.where(ok, yi * w + xi, torch.zeros_like(xi)).long()
        val = flat[:, lin.reshape(-1)].reshape(C, *ix.shape)
        out = out + torch.where(ok, val * wt, torch.zeros_like(val))
    return out


def reference(feats, cams, hyp, vis, G, dtype, pos=None):
    """feats = (ref [V,C,h,w], src [V,C,h,w]); cams [1,V+1,2,4,4]; hyp [1,D,h,w] or [1,D]; vis [V,h,w]; G [C,D,h,w].
    -> (g_ref [V,C,h,w], g_src [V,C,h,w], g_vis [V,h,w]) of sum(volume * G) in `dtype` (every view's term is differentiated on its
    own: the gradients are per view)."""
    ref, src = feats
    V, C, h, w = ref.shape
    pos = positions(cams, hyp, V, h, w) if pos is None else pos
    D = pos[0][0].shape[0]
    Gd = G.to(dtype).reshape(C, D, h * w)
    out = ([], [], [])
    for v in range(V):
        r, s, a = (t[v].detach().to(dtype).clone().requires_grad_(True) for t in (ref, src, vis))
        warped = bilinear(s, pos[v][0].to(dtype), pos[v][1].to(dtype))                     # [C, D, hw]
        vol = a.reshape(1, 1, h * w) * r.reshape(C, 1, h * w) * warped
        (vol * Gd).sum().backward()
        for o, t in zip(out, (r, s, a)):
            o.append(t.grad)
    return tuple(torch.stack(o) for o in out)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """((g_ref, g_src, g_vis) in float64, the same in float32) of a named case; cached, shared by every test of the case."""
    i = case_input(name)
    V, _, h, w = i["ref"].shape
    pos = positions(i["cams"], i["hyp"], V, h, w)
    return tuple(reference((i["ref"], i["src"]), i["cams"], i["hyp"], i["vis"], i["G"], dt, pos) for dt in (torch.float64, torch.float32))


# ------------------------------------------------------------------------------------------------
# the path model of the default (LDS box) kernel
# ------------------------------------------------------------------------------------------------
def kernel_constants(csrc=_CSRC):
    """{'TILE_X', 'TILE_Y', 'BOX', 'MIN_WGS', 'MIN_PLANES', 'MAX_VIEWS'} as the source text gives them: the tile of warp_common.hpp,
    the LDS box budget of warp_bwd.hip, the two numbers of its launcher's segment rule, the views of one launch (_lib.py)."""
    out = {}
    with open(os.path.join(csrc, "warp_common.hpp")) as f:
        text = f.read()
    for name in ("TILE_X", "TILE_Y"):
        m = re.search(r"^#define\s+CDS_%s\s+(\d+)\s*$" % name, text, re.M)
        assert m is not None, "CDS_%s not found: the box-plan model no longer knows the kernel's tile" % name
        out[name] = int(m.group(1))
    with open(os.path.join(csrc, "warp_bwd.hip")) as f:
        text = f.read()
    m = re.search(r"^#define\s+CDS_K3BWD_BOX\s+(\d+)\b", text, re.M)
    assert m is not None, "CDS_K3BWD_BOX not found: the box-plan model no longer knows the kernel's box budget"
    out["BOX"] = int(m.group(1))
    m = re.search(r"while \(base \* nseg < (\d+) && D / \(2 \* nseg\) >= (\d+)\) nseg \*= 2;\s*\n[^\n]*\n[^\n]*\n\s*hipLaunchKernelGGL\(warp_aggregate_bwd_box_kernel", text)
    assert m is not None, "the segment rule of the box kernel's launcher was not found: the box-plan model no longer knows it"
    out["MIN_WGS"], out["MIN_PLANES"] = int(m.group(1)), int(m.group(2))
    with open(os.path.join(os.path.dirname(csrc), "_lib.py")) as f:
        m = re.search(r"^MAX_VIEWS = (\d+)\s*$", f.read(), re.M)
    assert m is not None, "MAX_VIEWS not found"
    out["MAX_VIEWS"] = int(m.group(1))
    return out


def segments(V, C, D, h, w, k=None):
    """(nseg, planes per segment) of one launch over V <= MAX_VIEWS views, as cds_warp_aggregate_bwd_f32 chooses them (default kernel)."""
    k = k or kernel_constants()
    base = -(-w // k["TILE_X"]) * -(-h // k["TILE_Y"]) * V * (C // 8)
    nseg = 1
    while base * nseg < k["MIN_WGS"] and D // (2 * nseg) >= k["MIN_PLANES"]:
        nseg *= 2
    seg_planes = -(-D // nseg)
    return -(-D // seg_planes), seg_planes


def box_plan(cams, hyp, V, C, hw=None):
    """Texel count of the box of every workgroup of ONE channel group (each repeats C / 8 times), 0 = empty: no sample of the
    workgroup's (tile, view, depth segment) has a tap inside the source image.  The kernel's pass 1: the box spans the 2 x 2 cells of
    all samples with a tap inside, clipped to the image.  More than MAX_VIEWS views: the launches one after the other.
    hw = (h, w) is needed with shared hypotheses [1, D] only."""
    k = kernel_constants()
    h, w = hw if hw is not None else hyp.shape[2:]
    pos = positions(cams, hyp, V, h, w)
    D = pos[0][0].shape[0]
    out = []
    for v0 in range(0, V, k["MAX_VIEWS"]):
        nv = min(V, v0 + k["MAX_VIEWS"]) - v0
        nseg, seg_planes = segments(nv, C, D, h, w, k)
        for ty in range(0, h, k["TILE_Y"]):
            for tx in range(0, w, k["TILE_X"]):
                for v in range(v0, v0 + nv):
                    ix = pos[v][0].reshape(D, h, w)[:, ty:ty + k["TILE_Y"], tx:tx + k["TILE_X"]]
                    iy = pos[v][1].reshape(D, h, w)[:, ty:ty + k["TILE_Y"], tx:tx + k["TILE_X"]]
                    x0, y0 = torch.floor(ix), torch.floor(iy)
                    # a sample counts when one of its four taps is inside: x0 in [-1, w - 1] and y0 in [-1, h - 1]
                    any_in = (x0 >= -1) & (x0 <= w - 1) & (y0 >= -1) & (y0 <= h - 1)
                    for s in range(nseg):
                        sl = slice(s * seg_planes, min(D, (s + 1) * seg_planes))
                        m = any_in[sl]
                        if not bool(m.any()):
                            out.append(0)
                            continue
                        xs, ys = x0[sl][m].long(), y0[sl][m].long()
                        xmin, ymin = max(int(xs.min()), 0), max(int(ys.min()), 0)
                        xmax, ymax = min(int(xs.max()) + 1, w - 1), min(int(ys.max()) + 1, h - 1)
                        assert xmax >= xmin and ymax >= ymin
                        out.append((xmax - xmin + 1) * (ymax - ymin + 1))
    return out


def case_box_plan(name):
    i = case_input(name)
    V, C, h, w = i["ref"].shape
    return box_plan(i["cams"], i["hyp"], V, C, (h, w))


def mix(boxes, k=None):
    """'boxed / fallback / empty' counts of a plan (per channel group)."""
    k = k or kernel_constants()
    return (sum(1 for b in boxes if 0 < b <= k["BOX"]), sum(1 for b in boxes if b > k["BOX"]), sum(1 for b in boxes if b == 0))
