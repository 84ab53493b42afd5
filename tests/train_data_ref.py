"""Test infrastructure: numpy / PIL restatement of the reference's training datasets (datasets/dtu_yao.py, datasets/blended_dataset.py),
written from those two files independently of cds_mvsnet_amd.train_data, plus writers of tiny seeded dataset trees.

cv2 is not installed in this project's environment, so the reference's dataset modules cannot be imported: every cv2.resize(...,
INTER_NEAREST) is done with depth_eval_ref.nearest_index (OpenCV's documented index rule), and this restatement is UNCHECKED against a
run of the reference.  Where the reference leaves behaviour open - it shuffles the source views with the process-global numpy state -
the project's rule is restated instead: a permutation from np.random.default_rng([seed, epoch, index])."""
import os

import numpy as np
import torch

import depth_eval_ref as R

STAGES = ("stage1", "stage2", "stage3", "stage4")


# ---- the datasets -----------------------------------------------------------------------------------------------------------------
def read_pairs(path):
    with open(path) as f:
        num_viewpoint = int(f.readline())
        out = []
        for _ in range(num_viewpoint):
            ref_view = int(f.readline().rstrip())
            src_views = [int(x) for x in f.readline().rstrip().split()[1::2]]
            out.append((ref_view, src_views))
    return out


def scans_of(listfile):
    with open(listfile) as f:
        return [line.rstrip() for line in f.readlines()]


def dtu_metas(datapath, listfile):
    metas = []
    for scan in scans_of(listfile):
        for ref_view, src_views in read_pairs(os.path.join(datapath, "Cameras/pair.txt")):
            for light_idx in np.arange(7):
                metas.append((scan, int(light_idx), ref_view, list(src_views)))
    return metas


def blended_metas(datapath, listfile, nviews):
    metas = []
    for scan in scans_of(listfile):
        for ref_view, src_views in read_pairs(os.path.join(datapath, "{}/cams/pair.txt".format(scan))):
            if len(src_views) > 0:
                if len(src_views) < nviews:
                    src_views += [src_views[0]] * (nviews - len(src_views))
                metas.append((scan, ref_view, list(src_views)))
    return metas


def _matrix(lines, n):
    return np.array([float(x) for x in " ".join(lines).split()], dtype=np.float64).astype(np.float32).reshape(n, n)


def read_cam(filename, layout, ndepths, interval_scale):
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = _matrix(lines[1:5], 4)
    intrinsics = _matrix(lines[7:10], 3)
    depth_min = float(lines[11].split()[0])
    if layout == "dtu":
        depth_interval = float(lines[11].split()[1]) * interval_scale
    else:
        intrinsics[:2, :] /= 4.0
        depth_interval = float(lines[11].split()[1])
        if len(lines[11].split()) >= 3:
            num_depth = lines[11].split()[2]
            depth_max = depth_min + int(float(num_depth)) * depth_interval
            depth_interval = (depth_max - depth_min) / ndepths
        depth_interval *= interval_scale
    return intrinsics, extrinsics, depth_min, depth_interval


def depth_values(layout, depth_min, depth_interval, ndepths):
    if layout == "dtu":
        depth_max = depth_interval * ndepths + depth_min
    else:
        depth_max = depth_interval * (ndepths - 0.5) + depth_min
    return np.arange(depth_min, depth_max, depth_interval, dtype=np.float32)


def view_ids(layout, meta, mode, nviews, seed, epoch, index):
    ref_view, src_views = (meta[2], meta[3]) if layout == "dtu" else (meta[1], meta[2])
    src_views = list(src_views)
    if mode == "train":
        if layout == "blended":
            src_views = src_views[:7]
        perm = np.random.default_rng([seed, epoch, index]).permutation(len(src_views))
        src_views = [src_views[i] for i in perm]
    return [ref_view] + src_views[:(nviews - 1)]


def resize_nearest(a, w, h):
    """cv2.resize(a, (w, h), interpolation=cv2.INTER_NEAREST)."""
    return a[R.nearest_index(h, a.shape[0])][:, R.nearest_index(w, a.shape[1])]


def centre_crop(a, target_h, target_w):
    h, w = a.shape[:2]
    start_h, start_w = (h - target_h) // 2, (w - target_w) // 2
    return a[start_h: start_h + target_h, start_w: start_w + target_w]


def pyramid(a):
    h, w = a.shape
    return {"stage1": resize_nearest(a, w // 8, h // 8), "stage2": resize_nearest(a, w // 4, h // 4),
            "stage3": resize_nearest(a, w // 2, h // 2), "stage4": a}


def _read_pfm(path):
    from cds_mvsnet_amd import mvs_io                         # the file format reader is tested in test_mvs_io.py
    return np.array(mvs_io.read_pfm(path)[0], dtype=np.float32)


def sample(layout, datapath, metas, index, mode, nviews, ndepths, interval_scale, crop, seed=0, epoch=0):
    """One __getitem__: {imgs [N,3,h,w] float32, proj_matrices {stageK: [N,2,4,4]}, depth / mask {stageK}, depth_values, filename}."""
    from PIL import Image
    meta = metas[index]
    scan = meta[0]
    ids = view_ids(layout, meta, mode, nviews, seed, epoch, index)
    imgs, proj_matrices = [], []
    depth_ms = mask_ms = dv = None
    for i, vid in enumerate(ids):
        if layout == "dtu":
            img_filename = os.path.join(datapath, "Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, vid + 1, meta[1]))
            cam_filename = os.path.join(datapath, "Cameras/train/{:0>8}_cam.txt".format(vid))
            depth_filename = os.path.join(datapath, "Depths_raw/{}/depth_map_{:0>4}.pfm".format(scan, vid))
            mask_filename = os.path.join(datapath, "Depths_raw/{}/depth_visual_{:0>4}.png".format(scan, vid))
        else:
            img_filename = os.path.join(datapath, "{}/blended_images/{:0>8}.jpg".format(scan, vid))
            cam_filename = os.path.join(datapath, "{}/cams/{:0>8}_cam.txt".format(scan, vid))
            depth_filename = os.path.join(datapath, "{}/rendered_depth_maps/{:0>8}.pfm".format(scan, vid))
        np_img = np.array(Image.open(img_filename), dtype=np.float32) / 255.
        if layout == "blended":
            np_img = centre_crop(np_img, crop[0], crop[1])
        intrinsics, extrinsics, depth_min, depth_interval = read_cam(cam_filename, layout, ndepths, interval_scale)
        proj_mat = np.zeros(shape=(2, 4, 4), dtype=np.float32)
        proj_mat[0, :4, :4] = extrinsics
        proj_mat[1, :3, :3] = intrinsics
        proj_matrices.append(proj_mat)
        if i == 0:
            depth = _read_pfm(depth_filename)
            if layout == "dtu":
                mask = (np.array(Image.open(mask_filename), dtype=np.float32) > 10).astype(np.float32)
                h, w = depth.shape
                depth = centre_crop(resize_nearest(depth, w // 2, h // 2), crop[0], crop[1])
                mask = centre_crop(resize_nearest(mask, w // 2, h // 2), crop[0], crop[1])
            else:
                mask = centre_crop((depth > 0).astype(np.float32), crop[0], crop[1])
                depth = centre_crop(depth, crop[0], crop[1])
            depth_ms, mask_ms = pyramid(depth), pyramid(mask)
            dv = depth_values(layout, depth_min, depth_interval, ndepths)
        imgs.append(np_img)
    imgs = np.stack(imgs).transpose([0, 3, 1, 2])
    proj_matrices = np.stack(proj_matrices)
    ms = {}
    for name, s in zip(STAGES, (0.5, None, 2, 4)):
        m = proj_matrices.copy()
        if s is not None:
            m[:, 1, :2, :] = proj_matrices[:, 1, :2, :] * s
        ms[name] = m
    return {"imgs": imgs, "proj_matrices": ms, "depth": depth_ms, "depth_values": dv, "mask": mask_ms,
            "filename": scan + "/{}/" + "{:0>8}".format(ids[0]) + "{}"}


def collate(samples):
    """torch's default collate of the sample dicts -> tensors."""
    st = lambda xs: torch.from_numpy(np.stack([np.ascontiguousarray(x) for x in xs]))
    return {"imgs": st([s["imgs"] for s in samples]),
            "proj_matrices": {k: st([s["proj_matrices"][k] for s in samples]) for k in STAGES},
            "depth": {k: st([s["depth"][k] for s in samples]) for k in STAGES},
            "mask": {k: st([s["mask"][k] for s in samples]) for k in STAGES},
            "depth_values": st([s["depth_values"] for s in samples]),
            "filename": [s["filename"] for s in samples]}


# ---- tiny seeded trees --------------------------------------------------------------------------------------------------------------
def write_pairs(path, pairs):
    """pairs: [(ref, [src, ...])]; the score after each source id is a dummy, as the readers skip it."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("{}\n".format(len(pairs)))
        for ref, src in pairs:
            f.write("{}\n{}\n".format(ref, " ".join([str(len(src))] + ["{} {:.1f}".format(s, 100.0 - k) for k, s in enumerate(src)])))


def write_cam(path, extrinsic, intrinsic, depth_line):
    """mvs_io.write_cam_file, then the depth-range line replaced by ``depth_line`` (2, 3 or 4 values as text)."""
    from cds_mvsnet_amd import mvs_io
    cam = np.zeros((2, 4, 4), np.float32)
    cam[0], cam[1, :3, :3] = extrinsic, intrinsic
    os.makedirs(os.path.dirname(path), exist_ok=True)
    mvs_io.write_cam_file(path, cam)
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[11].split() == ["0.0"] * 4, lines
    lines[11] = depth_line
    with open(path, "w") as f:
        f.write("\n".join(lines))


def _cameras(n, H, W, seed, stage):
    from cds_mvsnet_amd import synth
    return synth.make_cameras(n, H, W, refine=True, seed=seed)[stage][0].numpy()


def _image(rs, H, W):
    """Smooth colour ramps plus noise, all byte values likely: survives JPEG without collapsing to a flat field."""
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(3 * x + 2 * y) % 256, (5 * y + x) % 256, (x * y) % 256], axis=-1)
    return ((base + rs.randint(0, 64, (H, W, 3))) % 256).astype(np.uint8)


def _depth(rs, H, W, holes):
    d = (500.0 + 250.0 * rs.rand(H, W)).astype(np.float32)
    if holes:
        d[rs.rand(H, W) < 0.3] = 0.0
    return d


def write_dtu_tree(root, scans=("scan1",), n_views=4, pairs=None, image_hw=(64, 96), gt_hw=(150, 210), seed=0,
                   depth_line="425.0 2.5"):
    """A DTU training tree: Cameras/pair.txt, Cameras/train/*_cam.txt, Rectified/{scan}_train/rect_*_{0..6}_r5000.png,
    Depths_raw/{scan}/depth_map_*.pfm + depth_visual_*.png.  -> the list file's path."""
    from PIL import Image
    from cds_mvsnet_amd import mvs_io
    rs = np.random.RandomState(seed)
    root = str(root)
    pairs = pairs if pairs is not None else [(v, [s for s in range(n_views) if s != v]) for v in range(n_views)]
    write_pairs(os.path.join(root, "Cameras/pair.txt"), pairs)
    cams = _cameras(n_views, 2 * image_hw[0], 2 * image_hw[1], seed, "stage2")   # the files hold the stage-2 intrinsics
    for v in range(n_views):
        write_cam(os.path.join(root, "Cameras/train/{:0>8}_cam.txt".format(v)), cams[v, 0], cams[v, 1, :3, :3], depth_line)
    for scan in scans:
        os.makedirs(os.path.join(root, "Rectified/{}_train".format(scan)), exist_ok=True)
        os.makedirs(os.path.join(root, "Depths_raw/{}".format(scan)), exist_ok=True)
        for v in range(n_views):
            for light in range(7):
                Image.fromarray(_image(rs, *image_hw)).save(
                    os.path.join(root, "Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, v + 1, light)))
            mvs_io.write_pfm(os.path.join(root, "Depths_raw/{}/depth_map_{:0>4}.pfm".format(scan, v)), _depth(rs, *gt_hw, holes=False))
            vis = np.where(rs.rand(*gt_hw) < 0.6, 255, rs.randint(0, 11, gt_hw)).astype(np.uint8)      # both sides of "> 10"
            Image.fromarray(vis).save(os.path.join(root, "Depths_raw/{}/depth_visual_{:0>4}.png".format(scan, v)))
    listfile = os.path.join(root, "list.txt")
    with open(listfile, "w") as f:
        f.write("".join(s + "\n" for s in scans))
    return listfile


def write_blended_tree(root, scans=("sceneA",), n_views=4, pairs=None, image_hw=(72, 104), seed=0, depth_lines=None,
                       listname="list.txt"):
    """A BlendedMVS tree: {scan}/cams/pair.txt, {scan}/cams/*_cam.txt, {scan}/blended_images/*.jpg, {scan}/rendered_depth_maps/*.pfm.
    depth_lines: per view, the camera file's line 11 (default: the four-value form mvs_io writes).  -> the list file's path."""
    from PIL import Image
    from cds_mvsnet_amd import mvs_io
    rs = np.random.RandomState(seed)
    root = str(root)
    for scan in scans:
        p = pairs if pairs is not None else [(v, [s for s in range(n_views) if s != v]) for v in range(n_views)]
        write_pairs(os.path.join(root, "{}/cams/pair.txt".format(scan)), p)
        cams = _cameras(n_views, image_hw[0], image_hw[1], seed, "stage4")           # the files hold the full-size intrinsics
        os.makedirs(os.path.join(root, "{}/blended_images".format(scan)), exist_ok=True)
        os.makedirs(os.path.join(root, "{}/rendered_depth_maps".format(scan)), exist_ok=True)
        for v in range(n_views):
            line = depth_lines[v] if depth_lines is not None else "425.0 2.5 128 745.0"
            write_cam(os.path.join(root, "{}/cams/{:0>8}_cam.txt".format(scan, v)), cams[v, 0], cams[v, 1, :3, :3], line)
            Image.fromarray(_image(rs, *image_hw)).save(os.path.join(root, "{}/blended_images/{:0>8}.jpg".format(scan, v)), quality=90)
            mvs_io.write_pfm(os.path.join(root, "{}/rendered_depth_maps/{:0>8}.pfm".format(scan, v)), _depth(rs, *image_hw, holes=True))
    listfile = os.path.join(root, listname)
    with open(listfile, "w") as f:
        f.write("".join(s + "\n" for s in scans))
    return listfile
