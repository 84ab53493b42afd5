"""Capture G15: the files the REFERENCE's colmap2mvsnet.py writes for a small COLMAP model.

Run in the build container only (``/root/reference`` is not present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_colmap.py

The reference script is compiled from the file where it lies (its ``import cv2`` / ``import multiprocessing`` lines and its
``__main__`` block left out); nothing of it is copied.  Stand-ins at capture time only: ``mp.Pool`` runs serially in this
process, ``np`` is a proxy of numpy that also has the removed ``asscalar``, and ``cv2`` is a name that is never called (every
image of the model is a ``.jpg``, which the reference copies).  A 12-image / 400-point model of
``synth.make_colmap_model`` (non-contiguous ids, -1 observations, duplicated observations, two camera models, one nearly
isolated image) is written as ``.txt`` and as ``.bin`` with the package's ``write_model``; the reference's own reader reads
it, and ``processing_single_scene`` converts it with max_d = 192 and max_d = 0 from either format.  Stored: the bytes of the
model files, of the input images and of every file the reference wrote (data only)."""
import argparse
import ast
import contextlib
import io
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import colmap_ref as R  # noqa: E402
from cds_mvsnet_amd import colmap, synth  # noqa: E402

REF = "/root/reference/colmap2mvsnet.py"
SEED = 15
MODEL = dict(n_images=12, n_points=400, mean_track=3.0, long_frac=0.02, n_isolated=1, invalid_frac=0.03, dup_frac=0.02,
             width=48, height=32, decimals=1)


class _NumpyWithAsscalar:
    asscalar = staticmethod(lambda a: a.item())

    def __getattr__(self, name):
        return getattr(np, name)


class _SerialPool:
    def __init__(self, processes=None):
        pass

    def map(self, fn, items):
        return [fn(x) for x in items]


class _SerialMp:
    Pool = _SerialPool
    cpu_count = staticmethod(lambda: 1)


def reference_module():
    """The reference script's globals, built from its own source at capture time."""
    with open(REF) as f:
        tree = ast.parse(f.read(), filename=REF)
    body = []
    for node in tree.body:
        if isinstance(node, ast.Import) and node.names[0].name in ("cv2", "multiprocessing"):
            continue
        if isinstance(node, ast.If):                       # the __main__ block
            continue
        body.append(node)
    glb = {"__builtins__": __builtins__, "__name__": "reference_colmap2mvsnet"}
    exec(compile(ast.Module(body=body, type_ignores=[]), REF, "exec"), glb)
    glb.update(np=_NumpyWithAsscalar(), mp=_SerialMp(), cv2=None)
    return glb


def tree_bytes(folder):
    out = {}
    for dirpath, _, files in os.walk(folder):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, folder).replace(os.sep, "/")] = open(p, "rb").read()
    return out


def pack_files(files, prefix):
    names = sorted(files)
    blob = b"".join(files[k] for k in names)
    offsets = np.cumsum([0] + [len(files[k]) for k in names]).astype(np.int64)
    return {f"{prefix}_names": np.array(names), f"{prefix}_offsets": offsets, f"{prefix}_blob": np.frombuffer(blob, np.uint8)}


def write_images(folder, images, width, height, rs):
    from PIL import Image
    os.makedirs(folder)
    ys, xs = np.mgrid[0:height, 0:width]
    for im in images.values():
        a, b, c = rs.uniform(0.1, 0.5, 3)
        img = np.stack([np.sin(a * xs + b * ys), np.cos(b * xs - c * ys), np.sin(c * xs) * np.cos(a * ys)], -1) * 100 + 128
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(folder, im.name), quality=75)


def g15_colmap():
    ref = reference_module()
    cameras, images, points = synth.make_colmap_model(seed=SEED, **MODEL)
    tmp = tempfile.mkdtemp()
    dense = os.path.join(tmp, "dense")
    write_images(os.path.join(dense, "images"), images, MODEL["width"], MODEL["height"], np.random.RandomState(SEED))
    sparse = os.path.join(dense, "sparse")
    colmap.write_model(sparse, ".txt", cameras, images, points)
    colmap.write_model(sparse, ".bin", cameras, images, points)
    # the reference's own readers see the model the package wrote
    for ext in (".txt", ".bin"):
        rc, ri, rp = ref["read_model"](sparse, ext)                                     # reference
        assert sorted(rc) == sorted(cameras) and sorted(ri) == sorted(images) and sorted(rp) == list(points.ids)
        for k, im in images.items():
            assert np.array_equal(ri[k].point3D_ids, im.point3D_ids) and np.array_equal(ri[k].xys, im.xys)
            assert np.array_equal(ri[k].qvec, im.qvec) and np.array_equal(ri[k].tvec, im.tvec) and ri[k].name == im.name
        for k, pid in enumerate(points.ids):
            assert np.array_equal(rp[pid].xyz, points.xyz[k]) and np.array_equal(rp[pid].image_ids, points.track(k)[0])
    arrays = {"seed": np.array(SEED), **pack_files({k: v for k, v in tree_bytes(dense).items() if k.startswith("sparse/")}, "model"),
              **pack_files({k: v for k, v in tree_bytes(dense).items() if k.startswith("images/")}, "images")}
    n_ties = 0
    for ext in (".txt", ".bin"):
        for max_d in (192, 0):
            save = os.path.join(tmp, f"scene{ext[1:]}{max_d}")
            os.makedirs(save)
            args = argparse.Namespace(dense_folder=dense, save_folder=save, max_d=max_d, interval_scale=1.0, theta0=5.0,
                                      sigma1=1.0, sigma2=10.0, model_ext=ext)
            with contextlib.redirect_stdout(io.StringIO()):
                ref["processing_single_scene"](args)                                     # reference
            files = tree_bytes(save)
            ties = []
            for row, (ids, scores) in enumerate(R.parse_pair(files["pair.txt"].decode())):
                assert np.isfinite(scores).all(), "a reference score is not finite: change the seed"
                for s in np.unique(scores):
                    if (scores == s).sum() > 1:
                        ties += [(row, k) for k in np.array(ids)[scores == s]]
            n_ties += len(ties)
            run = f"out_{ext[1:]}_{max_d}"
            arrays.update(pack_files(files, run))
            arrays[run + "_tied_ids"] = np.array(ties, np.int64).reshape(-1, 2)       # (row, id) of every listed tied score
    assert n_ties > 0, "no tied scores among the listed entries: the tie rule would go untested"
    shutil.rmtree(tmp)
    path = os.path.join(HERE, "g15_colmap.npz")
    np.savez_compressed(path, **arrays)
    print(f"g15_colmap: {os.path.getsize(path) / 1e3:.1f} KB, {n_ties} tied entries")


if __name__ == "__main__":
    g15_colmap()
