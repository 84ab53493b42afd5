"""A CPU model of the depth march of K3 / K1 (csrc/warp_lds.hip): which LDS chunks (d0, d1, staged) every workgroup walks through.

Written from the kernel's comments and the oracle's sample positions, NOT by calling the library.  It is only ever used as a
PRECONDITION on test inputs ("this input really contains N halved chunks"); it never decides whether an output is right.  At rounding
boundaries (a sample position within an ulp of a texel edge, a box of exactly the budget) it may differ from the kernel by a chunk or
two, which is why the tests ask for counts with a wide margin.

The rule modelled (warp_aggregate_lds_kernel / warp_entropy_lds_kernel):
  * cell of a sample = floor(position), clamped to [-2, n], NaN -> -2                                   (cell_of)
  * per pixel, the chunk's SMALLEST and LARGEST hypothesis give two cells; a view's box over the active pixels of a 32x8 tile is
    bw = xmax + 2 - xmin, bh = ymax + 2 - ymin, staged iff bw * bh <= cap                              (chunk_depth_range, reduce_boxes)
  * d1 = min(seg_end, d0 + dc); while some view of the launch does not fit and d1 - d0 > 8: d1 = d0 + ((((d1 - d0) >> 1) + 1) & ~1);
    the next chunk starts at d1.
The constants come from the source text of warp_lds.hip, so a retuned box budget changes the model with the kernel.
"""
import collections
import os
import re

import torch

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cds_mvsnet_amd", "csrc", "warp_lds.hip")


def kernel_constants(path=_SRC):
    """{'K3_TW', 'K3_TH', 'K3_BOX', 'K3_DC', 'K1_DC', 'K1_BOX'} as the #defines of warp_lds.hip give them."""
    with open(path) as f:
        text = f.read()
    out = {}
    for name in ("K3_TW", "K3_TH", "K3_BOX", "K3_DC", "K1_DC", "K1_BOX"):
        m = re.search(r"^#define\s+CDS_%s\s+(\d+)\s*$" % name, text, re.M)
        assert m is not None, "CDS_%s not found in %s: the chunk-plan model no longer knows the kernel's geometry" % (name, path)
        out[name] = int(m.group(1))
    return out


def k3_constants():
    c = kernel_constants()
    return dict(dc=c["K3_DC"], cap=c["K3_BOX"], tile=(c["K3_TW"], c["K3_TH"]))


def k1_constants(C):
    """K1 at C = 8 has its own chunk length and box budget; C = 16 / 32 use K3's."""
    c = kernel_constants()
    if C == 8:
        return dict(dc=c["K1_DC"], cap=c["K1_BOX"], tile=(c["K3_TW"], c["K3_TH"]))
    return k3_constants()


def k3_seg_planes(D, dc, ntiles, ngroups, nseg_env=None):
    """Planes per depth segment as cds_warp_aggregate_lds_launch chooses them (nseg_env: the value of CDS_K3_NSEG, None = unset)."""
    chunks = -(-D // dc)
    nseg = 1
    while nseg < chunks and ntiles * ngroups * nseg * 4 < 10 * 1024:
        nseg *= 2
    nseg = min(nseg, chunks)
    if nseg_env is not None and int(nseg_env) > 0:
        nseg = min(int(nseg_env), chunks)
    return -(-chunks // nseg) * dc


def cells_of_positions(ix, iy, h, w):
    def cell(p, n):
        c = torch.floor(p)
        c = torch.where(c >= -2.0, c, torch.full_like(c, -2.0))   # also NaN -> -2
        return torch.minimum(c, torch.full_like(c, float(n))).to(torch.int64)
    return cell(ix, w), cell(iy, h)


def sample_cells(cams, hyp, view):
    """Integer cells (cx, cy), each [D, h, w], of source view `view` (camera index, >= 1) for hypotheses hyp [1, D, h, w]."""
    from oracle import cds_oracle as O
    _, D, h, w = hyp.shape
    M = O.relative_projection(O.compose_projection(cams[:, view]), O.compose_projection(cams[:, 0]))
    ix, iy = O.sample_positions(M, hyp, h, w)
    return cells_of_positions(ix.reshape(D, h, w), iy.reshape(D, h, w), h, w)


Plan = collections.namedtuple("Plan", "full halved_staged fallback total offgrid_starts lengths max_chunks_per_workgroup workgroups")


def _summary(workgroups, dc):
    allc = [c for wg in workgroups for c in wg]
    return Plan(full=sum(1 for c in allc if c[2] and not c[3]),
                halved_staged=sum(1 for c in allc if c[2] and c[3]),
                fallback=sum(1 for c in allc if not c[2]),
                total=len(allc),
                offgrid_starts=sum(1 for c in allc if c[0] % dc),
                lengths=collections.Counter(c[1] - c[0] for c in allc),
                max_chunks_per_workgroup=max(len(wg) for wg in workgroups),
                workgroups=[[(d0, d1, staged) for d0, d1, staged, _ in wg] for wg in workgroups])


def march(cells, hyp, dc, cap, seg_planes=None, tile=(32, 8), rows=None):
    """The chunk lists of one launch.  cells: list over the launch's views of (cx, cy) [D, h, w]; hyp [D, h, w].
    rows = (y0, y1): the launch covers only these reference rows (a row window; its tiles start at y0)."""
    D, h, w = hyp.shape
    y0, y1 = rows if rows is not None else (0, h)
    tw, th = tile
    seg_planes = D if seg_planes is None else seg_planes
    workgroups = []
    for ty in range(y0, y1, th):
        for tx in range(0, w, tw):
            ys, xs = slice(ty, min(ty + th, y1)), slice(tx, min(tx + tw, w))
            hyp_t = hyp[:, ys, xs]
            cells_t = [(cx[:, ys, xs], cy[:, ys, xs]) for cx, cy in cells]
            for s0 in range(0, D, seg_planes):
                s1 = min(D, s0 + seg_planes)
                chunks = []
                d0 = s0
                while d0 < s1:
                    d1 = min(s1, d0 + dc)
                    halved = False
                    while True:
                        lo = hyp_t[d0:d1].argmin(0, keepdim=True) + d0
                        hi = hyp_t[d0:d1].argmax(0, keepdim=True) + d0
                        fits = True
                        for cx, cy in cells_t:
                            xa, xb = cx.gather(0, lo), cx.gather(0, hi)
                            ya, yb = cy.gather(0, lo), cy.gather(0, hi)
                            bw = int(torch.maximum(xa, xb).max()) + 2 - int(torch.minimum(xa, xb).min())
                            bh = int(torch.maximum(ya, yb).max()) + 2 - int(torch.minimum(ya, yb).min())
                            fits = fits and bw * bh <= cap
                        if fits or d1 - d0 <= 8:
                            break
                        d1 = d0 + ((((d1 - d0) >> 1) + 1) & ~1)
                        halved = True
                    chunks.append((d0, d1, fits, halved))
                    d0 = d1
                workgroups.append(chunks)
    return _summary(workgroups, dc)


def chunk_plan(cams, hyp, views, dc, cap, seg_planes=None, tile=(32, 8), rows=None):
    """Plan of one launch over the source views `views` (camera indices >= 1) of cams [1, N, 2, 4, 4] for hyp [1, D, h, w]."""
    cells = [sample_cells(cams, hyp, v) for v in views]
    return march(cells, hyp[0], dc, cap, seg_planes, tile, rows)


def merge(plans):
    """Counts of several launches taken together (K1: one workgroup per (tile, view), i.e. one single-view plan per view)."""
    lengths = collections.Counter()
    for p in plans:
        lengths.update(p.lengths)
    return Plan(sum(p.full for p in plans), sum(p.halved_staged for p in plans), sum(p.fallback for p in plans),
                sum(p.total for p in plans), sum(p.offgrid_starts for p in plans), lengths,
                max(p.max_chunks_per_workgroup for p in plans), [wg for p in plans for wg in p.workgroups])


def k3_launch_views(views, split_env=None):
    """The view lists of the launches of one K3 call over the source views `views` (more than four: two launches, the second
    accumulating; CDS_K3_SPLIT as the launcher reads it)."""
    views = list(views)
    V = len(views)
    if V <= 4:
        return [views]
    v1 = (V + 1) // 2
    if split_env is not None:
        e = int(split_env)
        if 1 <= e <= 4 and e < V and V - e <= 4:
            v1 = e
    return [views[:v1], views[v1:]]


# ------------------------------------------------------------------------------------------------
# The named inputs of tests/test_k3_depth_march_gpu.py (their preconditions are checked in tests/test_k3_chunk_plan_cpu.py)
# ------------------------------------------------------------------------------------------------
A_DEPTHS = (96, 97, 120, 145, 192, 194)
B_DEPTH = 145
N_SRC = 7            # source views every input provides (K3 takes up to 7 in two launches)
W_SHAPE = (3, 40, 40, 130)     # input W: V, D, h, w


def local_permutation(hyp, group, seed):
    """hyp [1, D, h, w] with every run of `group` consecutive planes shuffled independently per pixel: non-monotone hypotheses whose
    range over a chunk stays that of the ordered ones (a full permutation makes every chunk's range the whole sweep: all fallback.
    That case is input "W" below, run by test_k3_k1_wild_geometry_w_vs_oracle; test_warp_lds_fallbacks_wild_geometry of
    test_hip_parity.py does NOT cover it: every sample of its input lies outside every source image, so it compares zeros)."""
    g = torch.Generator().manual_seed(seed)
    D = hyp.shape[1]
    key = (torch.arange(D) // group).view(1, D, 1, 1).float() + 0.999 * torch.rand(hyp.shape, generator=g)
    return hyp.gather(1, key.argsort(1)).contiguous()


def named_input(name, D=B_DEPTH):
    """(cams [1, 8, 2, 4, 4], hyp [1, D, h, w]) of an input family.
    A / A2: friendly geometry (no chunk is ever halved), a long march; A2's width and height are no tile multiples.
    B: halving geometry (wider baseline, near depths); Bperm: B with locally permuted hypotheses.
    cfg4 / cfg4near: stage 1 of BASELINE config 4 (480x264, D = 48), default and near hypothesis range.
    W: wild geometry whose samples still hit the source images (cams [1, 4, 2, 4, 4], 40x130, D = 40): a wide baseline, hypotheses
    drawn independently per pixel and plane (every chunk spans the whole sweep: nearly all of K3's / K1's chunks take the global-memory
    path, and most workgroups of the K3 backward overflow their LDS box), and a third view whose z = 0 plane cuts the sweep."""
    from cds_mvsnet_amd import synth
    if name == "W":
        assert D == W_SHAPE[1]
        V, _, h, w = W_SHAPE
        cams = synth.make_cameras(V + 1, h, w, refine=False, seed=91, baseline=(150., 60., 15.))["stage3"]
        cams[0, 3, 0, :3, 3] += torch.tensor([0., 0., -600.])      # view 3: its z = 0 plane cuts the sweep (pz < 0 for about half of its samples)
        hyp = 300. + 600. * torch.rand(1, D, h, w, generator=torch.Generator().manual_seed(91))   # unordered per pixel
        return cams, hyp
    if name in ("A", "A2"):
        h, w = (24, 136) if name == "A" else (21, 77)
        return synth.stage_cameras(N_SRC + 1, h, w, seed=52), synth.make_hypotheses(D, h, w, seed=53)
    if name in ("B", "Bperm"):
        h, w = 64, 160
        assert D == B_DEPTH
        cams = synth.make_cameras(N_SRC + 1, h, w, seed=7, baseline=(80., 60., 15.))["stage3"]   # the first 7 cameras are those of make_cameras(7, ...)
        hyp = synth.make_hypotheses(D, h, w, lo=150., hi=902.5, seed=9)
        return cams, (local_permutation(hyp, 3, 13) if name == "Bperm" else hyp)
    if name in ("cfg4", "cfg4near"):
        h, w = 264, 480
        assert D == 48
        return synth.stage_cameras(7, h, w, seed=62), synth.make_hypotheses(D, h, w, lo=425. if name == "cfg4" else 300., seed=63)
    raise KeyError(name)


def w_features(C):
    """The feature pairs of input W at C channels (synth.make_pair_features layout, one pair per source view)."""
    from cds_mvsnet_amd import synth
    V, _, h, w = W_SHAPE
    return synth.make_pair_features(V, C, h, w, seed=91, sharp=True)


def assert_wild_input(name="W"):
    """The preconditions of the wild-geometry forward tests, as properties of the input: at least 90 % of K3's chunks and 60 % of K1's
    (C = 8) on the global-memory path, and the samples still inside the source images: all four taps for at least half of the samples
    of views 1 and 2 and for 5 % of the pole view's."""
    V, D = W_SHAPE[:2]
    cams, hyp = named_input(name, D)
    k = k3_constants()
    for views in ((1, 2, 3), (1, 2)):
        p = named_plan(name, D, views, k["dc"], k["cap"])
        assert p.fallback >= 0.9 * p.total, (name, views, p[:5])
    k = k1_constants(8)
    p = merge([named_plan(name, D, [v], k["dc"], k["cap"]) for v in range(1, V + 1)])
    assert p.fallback >= 0.6 * p.total, (name, "K1", p[:5])
    frac = [in_image_fraction(cams, hyp, v) for v in range(1, V + 1)]
    assert frac[0] >= 0.5 and frac[1] >= 0.5 and frac[2] >= 0.05, frac
    return frac


def in_image_fraction(cams, hyp, view):
    """Share of the samples of `view` whose four taps all lie inside the source image."""
    _, _, h, w = hyp.shape
    cx, cy = sample_cells(cams, hyp, view)
    return float(((cx >= 0) & (cx < w - 1) & (cy >= 0) & (cy < h - 1)).float().mean())


_PLAN_CACHE = {}


def named_plan(name, D, views, dc, cap, seg_planes=None):
    key = (name, D, tuple(views), dc, cap, seg_planes)
    if key not in _PLAN_CACHE:
        cams, hyp = named_input(name, D)
        _PLAN_CACHE[key] = chunk_plan(cams, hyp, views, dc, cap, seg_planes)
    return _PLAN_CACHE[key]


def assert_halving_input(name, D, views):
    """The preconditions of a B-family K3 launch over `views`, as properties of the input (one depth segment): at least 25 % of the
    chunks halved and staged, at most 15 % on the global-memory path, some workgroup marching >= 6 chunks."""
    k = k3_constants()
    p = named_plan(name, D, views, k["dc"], k["cap"])
    assert p.halved_staged >= 0.25 * p.total, (name, views, p[:5])
    assert p.fallback <= 0.15 * p.total, (name, views, p[:5])
    assert p.max_chunks_per_workgroup >= 6, (name, views, p.max_chunks_per_workgroup)
    return p


def assert_k1_halving_input(name, D, views, C):
    """K1 marches one view per workgroup with its own constants at C = 8: at least 10 % of all chunks halved and staged."""
    k = k1_constants(C)
    p = merge([named_plan(name, D, [v], k["dc"], k["cap"]) for v in views])
    assert p.halved_staged >= 0.10 * p.total, (name, views, C, p[:5])
    assert p.fallback <= 0.15 * p.total, (name, views, C, p[:5])
    return p
