"""numpy restatement of the evaluation-side image work, for the tests of cds_mvsnet_amd.eval_data / csrc/eval_data.hip.

* :func:`taps`: OpenCV's float32 INTER_LINEAR tap table along one axis (modules/imgproc/src/resize.cpp, the generic path:
  ``scale = 1. / (dst / src)`` in double, ``fx = (float)((dx + 0.5) * scale - 0.5)``, ``sx = cvFloor(fx)``, ``fx -= sx``, ``sx < 0`` and
  ``sx >= src - 1`` clamp the tap and zero the weight), written as a plain loop.
* :func:`resize`: HResizeLinear then VResizeLinear in a chosen dtype, every product and sum rounded to that dtype on its own
  (numpy never fuses), on the float32 ``u8 / 255`` image edge-padded by ``pad`` rows.
* :func:`outputs`: the host arithmetic of ``mvs_io.save_outputs``.
* :func:`write_scene`: a small MVSNet-format scene with uniformly random pixels.

cv2 is not installed here: this is a second restatement, not a run of OpenCV."""
import math
import os

import numpy as np


def taps(S, d):
    """-> (s0 [d] int64, s1 [d] int64, f [d] float32) for a source of S samples resized to d."""
    scale = 1.0 / (d / S)
    s0, s1, f = np.zeros(d, np.int64), np.zeros(d, np.int64), np.zeros(d, np.float32)
    for x in range(d):
        fx = np.float32((x + 0.5) * scale - 0.5)
        sx = int(math.floor(float(fx)))
        fx = np.float32(fx - np.float32(sx))
        if sx < 0:
            sx, fx = 0, np.float32(0)
        if sx >= S - 1:
            sx, fx = S - 1, np.float32(0)
        s0[x], s1[x], f[x] = sx, min(sx + 1, S - 1), fx
    return s0, s1, f


def prepared(u8, pad=0):
    """uint8 [Hs,Ws,3] -> the float32 image the reference resizes: / 255, then the Tanks & Temples edge rows."""
    img = np.array(u8, dtype=np.float32) / 255.
    if pad:
        img = np.pad(img, ((pad, pad), (0, 0), (0, 0)), "edge")
    return img


def resize(u8, h, w, pad=0, dtype=np.float32):
    """uint8 [Hs,Ws,3] -> [3,h,w] in ``dtype``: horizontal pass first, then vertical, on the float32 prepared image."""
    img = prepared(u8, pad).astype(dtype)
    r0, r1, fy = taps(img.shape[0], h)
    c0, c1, fx = taps(img.shape[1], w)
    fx, fy = fx.astype(dtype)[None, :, None], fy.astype(dtype)[:, None, None]
    one = dtype(1)
    rows = img[:, c0] * (one - fx) + img[:, c1] * fx                    # [Hp, w, 3]
    out = rows[r0] * (one - fy) + rows[r1] * fy                         # [h, w, 3]
    assert out.dtype == dtype
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def resize_through(u8, rows, cols, dtype=np.float32):
    """The two passes of :func:`resize` through GIVEN tap tables (rows, cols = (tap 0, tap 1, weight) that index the UNPADDED image,
    the form ``eval_data.linear_tables`` returns with the padding folded in): uint8 [Hs,Ws,3] -> [3,h,w] in ``dtype``."""
    img = prepared(u8).astype(dtype)
    (r0, r1, fy), (c0, c1, fx) = rows, cols
    fx, fy = np.asarray(fx).astype(dtype)[None, :, None], np.asarray(fy).astype(dtype)[:, None, None]
    one = dtype(1)
    line = img[:, c0] * (one - fx) + img[:, c1] * fx
    out = line[r0] * (one - fy) + line[r1] * fy
    assert out.dtype == dtype
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def outputs(confs, img_chw, h, w):
    """-> (conf3 [h,w,3] float32, img_u8 [h,w,3]): mvs_io.save_outputs's arrays (test.py:232-243)."""
    def nearest(a):
        H, W = a.shape[:2]
        ys = np.minimum((np.arange(h) * (H / h)).astype(np.int64), H - 1)
        xs = np.minimum((np.arange(w) * (W / w)).astype(np.int64), W - 1)
        return a[ys][:, xs]
    conf3 = np.ascontiguousarray(np.stack([nearest(c.astype(np.float32)) for c in confs], axis=-1))
    img = nearest(np.transpose(img_chw, (1, 2, 0)))
    return conf3, np.clip(img * 255, 0, 255).astype(np.uint8)


def random_u8(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def write_scene(root, scan, n_views, H, W, seed=0, quality=95):
    """<root>/<scan>/{images/%08d.jpg, cams/%08d_cam.txt, pair.txt}: uniformly random pixels, the cameras of synth.make_cameras;
    every view pairs with all the others."""
    from PIL import Image
    from cds_mvsnet_amd import synth
    cams = synth.make_cameras(n_views, H, W, refine=False, seed=seed)["stage3"][0].numpy()
    os.makedirs(os.path.join(root, scan, "images"))
    os.makedirs(os.path.join(root, scan, "cams"))
    for v in range(n_views):
        Image.fromarray(random_u8((H, W, 3), seed * 100 + v)).save(os.path.join(root, scan, "images", f"{v:08d}.jpg"), quality=quality)
        with open(os.path.join(root, scan, "cams", f"{v:08d}_cam.txt"), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(f"{x:.8f}" for x in r) for r in cams[v, 0]) + "\n\nintrinsic\n")
            f.write("\n".join(" ".join(f"{x:.8f}" for x in r[:3]) for r in cams[v, 1, :3]) + "\n\n425.0 2.5\n")
    with open(os.path.join(root, scan, "pair.txt"), "w") as f:
        f.write(f"{n_views}\n")
        for v in range(n_views):
            others = [u for u in range(n_views) if u != v]
            f.write(f"{v}\n{len(others)} " + " ".join(f"{u} {100.0 - u:.1f}" for u in others) + "\n")


def decoded(root, scan, vid):
    """The bytes PIL decodes for one view of :func:`write_scene`."""
    from PIL import Image
    with Image.open(os.path.join(root, scan, "images", f"{vid:08d}.jpg")) as im:
        return np.asarray(im.convert("RGB"))
