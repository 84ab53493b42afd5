"""Measurements behind profiles/train_from_disk.md: the loader of cds_mvsnet_amd.train_data and the epoch loop of cds_mvsnet_amd.fit on a
synthetic, seeded dataset tree at the real sizes (Blended: 768 x 576 JPEG, 5 views; DTU: 640 x 512 PNG with 1600 x 1200 ground truth).

    python scripts/time_train_from_disk.py tree   --root DIR           write the two trees (tests/train_data_ref.py's writers)
    python scripts/time_train_from_disk.py kernel                      ops.image_batch at both sizes (run it under rocprofv3 --kernel-trace --stats)
    python scripts/time_train_from_disk.py loader --root DIR           batches/s of TrainBatches alone, ahead=2 and ahead=0, next to the
                                                                       reference's host path (float /255, crop, stack, transpose, .to(device))
    python scripts/time_train_from_disk.py fit    --root DIR [--graph] time per step of fit() next to train_step on one resident sample

The images are colour ramps plus noise: noise decodes SLOWER than photographs (more entropy-coded bits per pixel), so the decode figures
are on the pessimistic side.  Every window is device-synchronised at both ends and timed on the host clock."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_data_ref as TR  # noqa: E402
from cds_mvsnet_amd import CDSMVSNet, fit, ops, seeded_init_  # noqa: E402
from cds_mvsnet_amd import train as T  # noqa: E402
from cds_mvsnet_amd import train_data as TD  # noqa: E402

DEV = "cuda"
SIZES = {"blended": (5, 576, 768), "dtu": (5, 512, 640)}
N = 5


def say(**kw):
    print(json.dumps(kw), flush=True)


def cmd_tree(args):
    t0 = time.time()
    TR.write_blended_tree(os.path.join(args.root, "blended"), n_views=10, image_hw=(576, 768), seed=1)
    TR.write_dtu_tree(os.path.join(args.root, "dtu"), n_views=10, image_hw=(512, 640), gt_hw=(1200, 1600), seed=2)
    with open(os.path.join(args.root, "blended", "long.txt"), "w") as f:      # the same scan 20 times over: 200 metas for the fit windows
        f.write("sceneA\n" * 20)
    with open(os.path.join(args.root, "blended", "mid.txt"), "w") as f:       # 60 metas for the loader windows
        f.write("sceneA\n" * 6)
    say(what="tree", seconds=round(time.time() - t0, 1))


def datasets(root, listname="list.txt", mode="train"):
    b = TD.BlendedTrainScenes(os.path.join(root, "blended"), os.path.join(root, "blended", listname), mode, N, 192, 1.0)
    d = TD.DTUTrainScenes(os.path.join(root, "dtu"), os.path.join(root, "dtu", "list.txt"), mode, N, 192, 1.06)
    return {"blended": b, "dtu": d}


def cmd_kernel(args):
    for name, (n, h, w) in SIZES.items():
        src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=DEV)
        r, c = ops.index_tables(np.arange(h), np.arange(w), h, w, DEV)
        for _ in range(5):
            ops.image_batch(src, r, c)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
        for a, b in ev:
            a.record()
            ops.image_batch(src, r, c)
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        nbytes = n * h * w * 3 * 5                                          # 1 byte read, 4 written per element
        say(what="kernel", size=name, shape=[n, h, w], bytes=nbytes, event_ms_median=ms[25], event_ms_min=ms[0],
            note="event brackets include launch gaps; the kernel's own time is in the rocprofv3 trace")


def reference_host_path(ds, index, epoch):
    """blended_dataset.py:86-92,165 / dtu_yao.py:73-77,176 for the images of one sample, then the upload."""
    from PIL import Image
    imgs = []
    for vid in ds.view_ids(index, epoch):
        a = np.array(Image.open(ds._paths(index, vid)["img"]), dtype=np.float32) / 255.
        if ds.layout == "blended":
            a = TR.centre_crop(a, *ds.crop)
        imgs.append(a)
    return torch.from_numpy(np.stack(imgs).transpose([0, 3, 1, 2])[None]).to(DEV)


def cmd_loader(args):
    for name, ds in datasets(args.root, "mid.txt").items():
        t0 = time.perf_counter()
        for i in range(10):
            ds.load(i, 0)
        say(what="decode", dataset=name, ms_per_sample_one_thread=round((time.perf_counter() - t0) * 100, 2))
        nb = len(TD.epoch_batches(len(ds), 1))
        for rep in range(3):
            row = {"what": "loader", "dataset": name, "repeat": rep, "batches": nb}
            for ahead in (2, 0):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with TD.TrainBatches(ds, 1, DEV, epoch=rep, threads=4, ahead=ahead) as it:
                    for s in it:
                        pass
                torch.cuda.synchronize()
                row[f"ahead{ahead}_batches_per_s"] = round(nb / (time.perf_counter() - t0), 1)
            order = TD.epoch_batches(len(ds), 1, epoch=rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in order:
                reference_host_path(ds, b[0], rep)
            torch.cuda.synchronize()
            row["reference_images_only_batches_per_s"] = round(nb / (time.perf_counter() - t0), 1)
            say(**row)
        # the stages of one batch, each on its own: copy, image prep, ground truth
        it = TD.TrainBatches(ds, 1, DEV, epoch=0, ahead=0)
        next(it)
        slot = it._ring[0]
        Hs, Ws, Hg, Wg = slot["sizes"]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        times = []
        for _ in range(20):
            ev[0].record()
            staged = slot["buf"].to(DEV, non_blocking=True)
            ev[1].record()
            img_tab, gt_tab = it._tables("img", Hs, Ws), it._tables("gt", Hg, Wg)
            ops.image_batch(staged[:N * Hs * Ws * 3].view(N, Hs, Ws, 3), *img_tab)
            ev[2].record()
            d = staged[slot["off_d"]:slot["off_d"] + 4 * Hg * Wg].view(torch.float32).view(Hg, Wg)
            m = staged[slot["off_m"]:slot["off_m"] + Hg * Wg].view(Hg, Wg) if slot["mask"] is not None else None
            ops.gt_pyramid(d, gt_tab[0], gt_tab[1], levels=4, mask_src=m)
            ev[3].record()
            torch.cuda.synchronize()
            times.append([ev[k].elapsed_time(ev[k + 1]) for k in range(3)])
        it.close()
        med = [statistics.median(t[k] for t in times) for k in range(3)]
        say(what="stages", dataset=name, staged_bytes=int(slot["buf"].numel()), copy_ms=round(med[0], 3), image_batch_ms=round(med[1], 3),
            gt_pyramid_ms=round(med[2], 3))


def cmd_fit(args):
    ds = datasets(args.root, "long.txt")["blended"]
    steps = len(TD.epoch_batches(len(ds), 1))
    model = seeded_init_(CDSMVSNet(refine=True, ndepths=(48, 32, 8), depth_interals_ratio=(4.0, 1.5, 0.75)), 0).to(DEV)
    with TD.TrainBatches(ds, 1, DEV, epoch=1, ahead=0) as it:
        resident = next(it)

    def window_fit():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        log = fit.fit(model, [ds], [], epochs=1, batch_size=1, logging_every=100, graph=args.graph, log=lambda s: None)
        torch.cuda.synchronize()
        assert log[0]["steps"] == steps
        return (time.perf_counter() - t0) * 1e3 / steps

    def window_resident():
        opt = T.make_optimizer(model)
        step = T.CapturedTrainStep(model, opt) if args.graph else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            if step is not None:
                loss, _ = step(resident, 1.0)
            else:
                loss, _ = T._step_tensors(model, opt, resident, 1.0, (0.5, 1.0, 2.0), None, None)
            if k % 100 == 0:
                float(loss)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    window_resident()                                          # warm-up: allocator, the backward's audit, attribute calls
    for rep in range(3):
        say(what="fit", graph=bool(args.graph), repeat=rep, steps=steps, fit_ms_per_step=round(window_fit(), 3),
            resident_ms_per_step=round(window_resident(), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["tree", "kernel", "loader", "fit"])
    ap.add_argument("--root", default=os.path.join(tempfile.gettempdir(), "cds_train_tree"))
    ap.add_argument("--graph", action="store_true")
    args = ap.parse_args()
    {"tree": cmd_tree, "kernel": cmd_kernel, "loader": cmd_loader, "fit": cmd_fit}[args.cmd](args)


if __name__ == "__main__":
    main()
