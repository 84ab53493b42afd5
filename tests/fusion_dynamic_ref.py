"""Torch restatement of the dynamic-consistency fusion rule (include/cds_mvsnet_hip.h), in float32 or float64.

Steps 1 and 2 are built exactly as ``oracle.cds_oracle.fuse_view`` builds them: ``_pixel_centres`` / ``_lift_and_project`` /
``confidence_mask`` and ``F.grid_sample(..., align_corners=True, padding_mode="zeros")``.  The float64 variant casts the
float32 inputs (pixel centres included); it measures how many pixels sit so close to a threshold that rounding decides them.

Also here: the five test scenes of the feature's tests (shared by the CPU and the GPU file) and their cached references.
"""
import functools

import torch
import torch.nn.functional as F

from cds_mvsnet_amd import synth
from oracle import cds_oracle as O

DIST_BASE = 0.25
REL_BASE = 1.0 / 1300.0
N_VIEWS = (2, 10)

# V, h, w, seed, amp, conf: odd sizes and partial workgroups; V < n_min, V = n_max, V > n_max; confidence-zeroed taps
CASES = [(1, 37, 53, 12, 12, (0.0, 0.0, 0.0)),
         (3, 37, 53, 14, 12, (0.05, 0.03, 0.02)),
         (7, 64, 80, 18, 12, (0.0, 0.0, 0.0)),
         (10, 48, 64, 21, 20, (0.05, 0.03, 0.02)),
         (12, 33, 47, 23, 20, (0.0, 0.0, 0.0))]
CASE_IDS = [f"V{c[0]}" for c in CASES]


@functools.lru_cache(maxsize=None)
def make_case(V, h, w, seed, amp):
    """synth.make_fusion_scene(V + 1, h, w, seed, outlier_frac=0.05) with every SOURCE depth multiplied by
    1 + u amp / 1300, u uniform in (-1, 1) per pixel: the relative depth errors spread over the levels."""
    sc = synth.make_fusion_scene(V + 1, h, w, seed=seed, outlier_frac=0.05)
    g = torch.Generator().manual_seed(seed + 1000)
    u = torch.rand(V, h, w, generator=g) * 2.0 - 1.0
    depths = sc["depths"].clone()
    depths[1:] = depths[1:] * (1.0 + u * (amp / 1300.0))
    return {"depths": depths, "confs": sc["confs"], "cams": sc["cams"], "imgs": sc["imgs"]}


def admit_from_levels(levels, n_min=N_VIEWS[0], n_max=N_VIEWS[1]):
    """Step 4.  levels [V, ...] integer (n_max + 1: inconsistent) -> admit [...] int64: the smallest n in
    [n_min, min(n_max, V)] with #{v : l_v <= n} >= n, or 0."""
    levels = torch.as_tensor(levels)
    V = levels.shape[0]
    admit = torch.zeros(levels.shape[1:], dtype=torch.int64)
    for n in range(min(n_max, V), n_min - 1, -1):       # descending: the smallest admitting n is written last
        admit = torch.where((levels <= n).sum(0) >= n, torch.full_like(admit, n), admit)
    return admit


def fuse_view_dynamic(ref_depth, ref_conf, ref_cam, src_depths, src_confs, src_cams, conf=(0.0, 0.0, 0.0),
                      dist_base=DIST_BASE, rel_base=REL_BASE, n_views=N_VIEWS, dtype=torch.float32):
    """One reference view, steps 1-7 -> {"depth", "mask", "points", "admit" int64 [h,w], "levels" int64 [V,h,w]}."""
    n_min, n_max = n_views
    ref_depth, ref_conf, ref_cam = ref_depth.to(dtype), ref_conf.to(dtype), ref_cam.to(dtype)
    src_depths, src_confs, src_cams = src_depths.to(dtype), src_confs.to(dtype), src_cams.to(dtype)
    h, w = ref_depth.shape
    V = src_depths.shape[0]
    pix = O._pixel_centres(h, w).to(dtype)
    db, rb = torch.tensor(dist_base, dtype=dtype), torch.tensor(rel_base, dtype=dtype)
    levels, reproj_d = [], []
    for v in range(V):
        sd = src_depths[v] * O.confidence_mask(src_confs[v], conf).to(dtype)
        xy_sr, d_sr = O._lift_and_project(pix, sd, src_cams[v], ref_cam)            # source pixel -> reference view
        xyd = torch.cat([xy_sr, d_sr.unsqueeze(-1)], -1).permute(2, 0, 1).unsqueeze(0)
        xy_rs, _ = O._lift_and_project(pix, ref_depth, ref_cam, src_cams[v])         # reference pixel -> source view
        grid = torch.stack([xy_rs[..., 0] / w, xy_rs[..., 1] / h], -1)
        grid = (grid * 2 - 1).clamp(-1.1, 1.1)
        inside = ((grid[..., 0] >= -1) & (grid[..., 0] <= 1) & (grid[..., 1] >= -1) & (grid[..., 1] <= 1))
        rep = F.grid_sample(xyd, grid.unsqueeze(0), mode="bilinear", padding_mode="zeros", align_corners=True)[0]
        e = (rep[:2] - pix[..., :2, 0].permute(2, 0, 1)).norm(dim=0)
        r = (ref_depth - rep[2]).abs() / ref_depth
        lv = torch.full((h, w), n_max + 1, dtype=torch.int64)
        for n in range(n_max, 0, -1):                                                # the smallest passing n is written last
            nf = torch.tensor(float(n), dtype=dtype)
            lv = torch.where(inside & (e < nf * db) & (r < nf * rb), torch.full_like(lv, n), lv)
        levels.append(lv)
        reproj_d.append(rep[2])
    levels, rz = torch.stack(levels), torch.stack(reproj_d)
    admit = admit_from_levels(levels, n_min, n_max)
    cons = levels <= n_max
    fused = ref_depth
    for v in range(V):                                                               # in view order
        fused = fused + torch.where(cons[v], rz[v], torch.zeros_like(rz[v]))
    fused = fused / (1 + cons.sum(0)).to(dtype)
    mask = (admit > 0) & O.confidence_mask(ref_conf, conf)
    ray = torch.inverse(ref_cam[1, :3, :3]) @ pix
    pc = ray / (ray[..., -1:, :] + 1e-9) * fused[..., None, None]
    pc = torch.cat([pc, torch.ones_like(pc[..., -1:, :])], -2)
    pw = torch.inverse(ref_cam[0]) @ pc
    pw = pw / (pw[..., -1:, :] + 1e-9)
    return {"depth": fused, "mask": mask.to(torch.float32), "points": pw[..., :3, 0].permute(2, 0, 1), "admit": admit,
            "levels": levels}


@functools.lru_cache(maxsize=None)
def case_reference(i, dtype=torch.float32, n_views=N_VIEWS, scale=1.0):
    """The reference of CASES[i] (cached: computed once per process, shared by the tests; do not modify the result)."""
    V, h, w, seed, amp, conf = CASES[i]
    sc = make_case(V, h, w, seed, amp)
    return fuse_view_dynamic(sc["depths"][0], sc["confs"][0], sc["cams"][0], sc["depths"][1:], sc["confs"][1:], sc["cams"][1:],
                             conf=conf, dist_base=DIST_BASE * scale, rel_base=REL_BASE * scale, n_views=n_views, dtype=dtype)
