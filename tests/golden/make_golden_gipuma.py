"""Capture G14: the files the REFERENCE's gipuma conversion writes for a small scan (gipuma.py:20-175).

Run in the build container only (``/root/reference`` is not present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gipuma.py

The reference's gipuma.py cannot be imported here (its ``from utils import *`` pulls in torchvision), so the functions are
compiled one by one from the reference file with ``make_golden._reference_function``; nothing is copied.  A 3-view 12x16
scan in the layout ``infer`` writes is converted by ``probability_filter`` and ``mvsnet_to_gipuma`` with nonzero thresholds,
and the bytes of every input and output file are stored (data only), with what ``read_gipuma_dmb`` returns for the two
``.dmb`` files of each view.
"""
import os
import re
import shutil
import struct
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (puts the repository and the reference on sys.path)

from cds_mvsnet_amd import mvs_io  # noqa: E402

REF = "/root/reference/gipuma.py"
PROB_THRESHOLD = (0.3, 0.2, 0.1)


def _reference_gipuma():
    env = {"os": os, "shutil": shutil, "pack": struct.pack, "unpack": struct.unpack}
    for name in ("read_pfm", "save_pfm"):
        env[name] = G._reference_function("/root/reference/datasets/data_io.py", name, {"re": re, "sys": sys})
    for name in ("read_camera_parameters", "read_gipuma_dmb", "write_gipuma_dmb", "mvsnet_to_gipuma_dmb", "mvsnet_to_gipuma_cam",
                 "fake_gipuma_normal", "mvsnet_to_gipuma", "probability_filter"):
        env[name] = G._reference_function(REF, name, env)     # each sees the ones compiled before it
    return env


def write_scan(folder, rs, n=3, h=12, w=16):
    from PIL import Image
    for sub in ("depth_est", "confidence", "cams", "images"):
        os.makedirs(os.path.join(folder, sub))
    for v in range(n):
        depth = (rs.rand(h, w) * 500 + 400).astype(np.float32)
        depth[rs.rand(h, w) < 0.1] = 0.0
        mvs_io.write_pfm(os.path.join(folder, "depth_est", f"{v:08d}.pfm"), depth)
        mvs_io.write_pfm(os.path.join(folder, "confidence", f"{v:08d}.pfm"), rs.rand(h, w, 3).astype(np.float32))
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0] = np.eye(4)
        cam[0, :3, :3] += (rs.rand(3, 3) - 0.5) * 0.1
        cam[0, :3, 3] = rs.rand(3) * 100 - 50
        cam[1, :3, :3] = [[14.4 + v, 0, 8.1], [0, 14.2 - v, 5.9], [0, 0, 1]]
        cam[1, 3, 3] = 1.0
        mvs_io.write_cam_file(os.path.join(folder, "cams", f"{v:08d}_cam.txt"), cam)
        Image.fromarray((rs.rand(h, w, 3) * 255).astype(np.uint8)).save(os.path.join(folder, "images", f"{v:08d}.jpg"))


def tree_bytes(folder):
    out = {}
    for dirpath, _, files in os.walk(folder):
        for fn in files:
            p = os.path.join(dirpath, fn)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


def pack_files(files, prefix):
    names = sorted(files)
    blob = b"".join(files[k] for k in names)
    offsets = np.cumsum([0] + [len(files[k]) for k in names]).astype(np.int64)
    return {f"{prefix}_names": np.array(names), f"{prefix}_offsets": offsets,
            f"{prefix}_blob": np.frombuffer(blob, np.uint8)}


def g14_gipuma_formats():
    ref = _reference_gipuma()
    rs = np.random.RandomState(14)
    tmp = tempfile.mkdtemp()
    scan = os.path.join(tmp, "scan1")
    write_scan(scan, rs)
    inputs = tree_bytes(scan)
    ref["probability_filter"](scan, list(PROB_THRESHOLD))                      # reference
    point_folder = os.path.join(scan, "points_mvsnet")
    os.mkdir(point_folder)                                                    # gipuma_filter creates it (gipuma.py:205-207)
    ref["mvsnet_to_gipuma"](scan, point_folder)                               # reference
    outputs = {k: v for k, v in tree_bytes(scan).items() if k not in inputs}
    reads = {}
    for v in range(3):
        for fn in ("disp", "normals"):
            reads[f"read_{fn}_{v}"] = ref["read_gipuma_dmb"](os.path.join(point_folder, f"2333__{v:08d}", fn + ".dmb"))
    shutil.rmtree(tmp)
    G.save("g14_gipuma_formats", prob_threshold=np.array(PROB_THRESHOLD), **pack_files(inputs, "in"),
           **pack_files(outputs, "out"), **reads)


if __name__ == "__main__":
    g14_gipuma_formats()
