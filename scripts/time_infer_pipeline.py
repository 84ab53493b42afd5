"""Measurements behind profiles/infer_pipeline.md: `infer --pipeline host` next to `--pipeline gpu` on synthetic, seeded scans at the
sizes of the reference's evaluation recipes.

    python scripts/time_infer_pipeline.py tree     --root DIR               write the two scans
    python scripts/time_infer_pipeline.py kernel                            ops.eval_views / ops.eval_outputs at both sizes (run it under
                                                                            rocprofv3 --kernel-trace --stats for the kernels' own times)
    python scripts/time_infer_pipeline.py host     --root DIR --scan dtu    the host-side stages of both pipelines on one thread, no GPU call:
                                                                            EvalScenes[i], save_outputs, one decode, the writer's files
    python scripts/time_infer_pipeline.py pipeline --root DIR --scan dtu    wall time per depth map, host and gpu alternating in one
                                                                            process, and the forward's own time on a resident sample

    dtu: 49 views, 1600 x 1200 JPEG, --max_h 1184 --max_w 1600 --num_view 5 (scripts/dtu_eval.sh)
    tt:  1080 x 1920 JPEG, --dataset tt --max_h 544 --max_w 1024 --num_view 11 --ndepths 64,32,8 --numdepth 256 (scripts/tt_eval.sh)

The images are colour ramps plus noise: noise decodes SLOWER than photographs, so the decode figures are on the pessimistic side.
Every window is device-synchronised at both ends and timed on the host clock; both pipelines write their files to --out."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cds_mvsnet_amd import infer, ops, synth  # noqa: E402
from cds_mvsnet_amd import eval_data as E  # noqa: E402
from cds_mvsnet_amd.mvs_io import EvalScenes  # noqa: E402

DEV = "cuda"
SCANS = {
    "dtu": dict(views=49, hw=(1200, 1600), sources=10,
                flags=["--max_h", "1184", "--max_w", "1600", "--num_view", "5"]),
    "tt": dict(views=24, hw=(1080, 1920), sources=10,
               flags=["--dataset", "tt", "--max_h", "544", "--max_w", "1024", "--num_view", "11", "--ndepths", "64,32,8", "--numdepth", "256"]),
}


def say(**kw):
    print(json.dumps(kw), flush=True)


def write_scan(root, scan, views, hw, sources, seed):
    from PIL import Image
    H, W = hw
    cams = synth.make_cameras(views, H, W, refine=False, seed=seed)["stage3"][0].numpy()
    os.makedirs(os.path.join(root, scan, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, scan, "cams"), exist_ok=True)
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    for v in range(views):
        ramp = np.stack([(xx * (v + 1) // 7) % 256, (yy * (v + 2) // 5) % 256, ((xx + yy) // 3 + 16 * v) % 256], axis=-1)
        img = np.clip(ramp + rs.randint(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, scan, "images", f"{v:08d}.jpg"), quality=95)
        with open(os.path.join(root, scan, "cams", f"{v:08d}_cam.txt"), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(f"{x:.8f}" for x in r) for r in cams[v, 0]) + "\n\nintrinsic\n")
            f.write("\n".join(" ".join(f"{x:.8f}" for x in r[:3]) for r in cams[v, 1, :3]) + "\n\n425.0 2.5\n")
    with open(os.path.join(root, scan, "pair.txt"), "w") as f:
        f.write(f"{views}\n")
        for v in range(views):                                 # the nearest view ids on either side, as a DTU pair file looks
            near = sorted((u for u in range(views) if u != v), key=lambda u: (abs(u - v), u))[:sources]
            f.write(f"{v}\n{len(near)} " + " ".join(f"{u} {100.0 - abs(u - v):.1f}" for u in near) + "\n")
    with open(os.path.join(root, f"{scan}.txt"), "w") as f:
        f.write(scan + "\n")


def cmd_tree(args):
    t0 = time.time()
    for i, (scan, c) in enumerate(SCANS.items()):
        write_scan(args.root, scan, c["views"], c["hw"], c["sources"], seed=i + 1)
    say(what="tree", seconds=round(time.time() - t0, 1))


def _events(fn, n=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)


def cmd_kernel(args):
    note = "event brackets include launch gaps; the kernel's own time is in the rocprofv3 trace"
    for name, V, (Hs, Ws), pad, (h, w) in (("dtu", 5, (1200, 1600), 0, (1184, 1600)), ("dtu-1", 1, (1200, 1600), 0, (1184, 1600)),
                                           ("tt", 11, (1080, 1920), 4, (544, 1024)), ("tt-1", 1, (1080, 1920), 4, (544, 1024))):
        src = torch.randint(0, 256, (V, Hs, Ws, 3), dtype=torch.uint8, device=DEV)
        rows, cols = E.view_tables(Hs, Ws, pad, h, w, DEV)
        ms = _events(lambda: ops.eval_views(src, rows, cols))
        say(what="eval_views", size=name, views=V, src=[Hs, Ws], pad=pad, out=[h, w], bytes=V * (Hs * Ws * 3 + h * w * 12),
            event_ms_median=ms[len(ms) // 2], event_ms_min=ms[0], note=note)
    for name, (h, w) in (("dtu", (1184, 1600)), ("tt", (544, 1024))):
        shapes = [(h // 4, w // 4), (h // 2, w // 2), (h, w), (h, w)]
        confs = [torch.rand(s, device=DEV) for s in shapes[:3]]
        img = torch.rand((3, h, w), device=DEV)
        tab = E.output_tables(shapes, h, w, DEV)
        ms = _events(lambda: ops.eval_outputs(confs, img, tab, h, w))
        say(what="eval_outputs", size=name, out=[h, w], bytes=h * w * (12 + 12 + 12 + 3), event_ms_median=ms[len(ms) // 2],
            event_ms_min=ms[0], note=note)


def cmd_host(args):
    """Median [min, max] of 5, one thread, files in the page cache after the first pass; nothing here touches the GPU."""
    from cds_mvsnet_amd import mvs_io
    c = SCANS[args.scan]
    a = infer.parse_args(["--testpath", args.root, "--testlist", "x", "--outdir", args.out, "--interval_scale", "1.0"] + c["flags"])
    data = EvalScenes(args.root, [args.scan], nviews=a.num_view, ndepths=a.numdepth, interval_scale=a.interval_scale, max_h=a.max_h,
                      max_w=a.max_w, refine=a.refine, dataset=a.dataset)

    def stat(fn):
        ts = []
        for i in range(5):
            t0 = time.perf_counter()
            fn(i)
            ts.append((time.perf_counter() - t0) * 1e3)
        return [round(statistics.median(ts), 1), round(min(ts), 1), round(max(ts), 1)]

    h, w = a.max_h, a.max_w
    rs = np.random.RandomState(0)
    depth = rs.rand(h, w).astype(np.float32)
    confs = [rs.rand(h // 4, w // 4).astype(np.float32), rs.rand(h // 2, w // 2).astype(np.float32), rs.rand(h, w).astype(np.float32)]
    img = data[0]["imgs"][0]
    cam = np.zeros((2, 4, 4), np.float32)
    conf3 = np.ascontiguousarray(np.stack([mvs_io.nearest_resize(x, h, w) for x in confs], -1))
    u8 = np.clip(mvs_io.nearest_resize(img.transpose(1, 2, 0), h, w) * 255, 0, 255).astype(np.uint8)
    path = os.path.join(args.root, args.scan, "images", "00000003.jpg")
    buf = np.empty(c["hw"] + (3,), np.uint8)
    out = os.path.join(args.out, "host_stages")
    shutil.rmtree(out, ignore_errors=True)
    say(what="host", scan=args.scan, views=a.num_view, unit="ms: median, min, max of 5",
        eval_scenes_getitem=stat(lambda i: data[i]),
        save_outputs=stat(lambda i: mvs_io.save_outputs(out, "s/{}/%08d{}" % i, depth, confs, cam, img)),
        decode_one_view=stat(lambda i: E._decode(path, buf)),
        writer_files=stat(lambda i: E._write_files(out, "t/{}/%08d{}" % i, depth, conf3, cam, u8, [])))
    shutil.rmtree(out, ignore_errors=True)


def cmd_pipeline(args):
    c = SCANS[args.scan]
    base = ["--testpath", args.root, "--testlist", os.path.join(args.root, f"{args.scan}.txt"), "--interval_scale", "1.0"] + c["flags"]
    a = infer.parse_args(base + ["--outdir", args.out])
    scene_args = dict(nviews=a.num_view, ndepths=a.numdepth, interval_scale=a.interval_scale, max_h=a.max_h, max_w=a.max_w,
                      refine=a.refine, dataset=a.dataset)
    dev = torch.device(DEV, 0)
    torch.cuda.set_device(dev)
    model = infer.build_model(a).to(dev).eval()
    scans = [args.scan]
    n = c["views"]

    # the forward on a resident sample: the bound for pipelines that cost nothing
    with E.EvalViews(args.root, scans, device=dev, ahead=0, **scene_args) as it:
        s = next(it)
    cams = {k: torch.from_numpy(v).unsqueeze(0) for k, v in s["proj_matrices"].items()}
    dv = torch.from_numpy(s["depth_values"]).unsqueeze(0)
    with torch.no_grad():
        ms = _events(lambda: model(s["imgs"], cams, dv, temperature=a.temperature), n=10, warm=3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            model(s["imgs"], cams, dv, temperature=a.temperature)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 100
    say(what="forward", scan=args.scan, event_ms_median=round(ms[5], 3), event_ms_min=round(ms[0], 3), event_ms_max=round(ms[-1], 3),
        wall_ms_back_to_back=round(wall, 3))

    # the host share of the host pipeline, stage by stage, one thread (median of 5 samples)
    data = EvalScenes(args.root, scans, **scene_args)
    t_item = []
    for idx in range(5):
        t0 = time.perf_counter()
        smp = data[idx]
        t1 = time.perf_counter()
        torch.from_numpy(smp["imgs"]).unsqueeze(0).to(dev)
        torch.cuda.synchronize()
        t_item.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
    say(what="host_stages", scan=args.scan, getitem_ms=round(statistics.median(t[0] for t in t_item), 2),
        upload_ms=round(statistics.median(t[1] for t in t_item), 2))

    for rep in range(args.repeats):
        row = {"what": "pipeline", "scan": args.scan, "repeat": rep, "depth_maps": n}
        for pipeline in ("host", "gpu"):
            out = os.path.join(args.out, f"{pipeline}{rep}")
            shutil.rmtree(out, ignore_errors=True)
            a = infer.parse_args(base + ["--outdir", out, "--pipeline", pipeline])
            last = "stage4" if a.refine else "stage3"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if pipeline == "host":
                times = infer._run_host_pipeline(a, model, EvalScenes(args.root, scans, **scene_args), dev, 0, 1, last)
                row["host_forward_window_ms"] = round(float(np.mean(times)) * 1e3, 2)      # upload + forward + synchronise, as infer prints it
            else:
                infer._run_gpu_pipeline(a, model, scans, scene_args, dev, 0, 1, last)
            torch.cuda.synchronize()
            row[f"{pipeline}_ms_per_depth_map"] = round((time.perf_counter() - t0) * 1e3 / n, 2)
            shutil.rmtree(out, ignore_errors=True)
        say(**row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["tree", "kernel", "host", "pipeline"])
    ap.add_argument("--root", default=os.path.join(tempfile.gettempdir(), "cds_eval_tree"))
    ap.add_argument("--out", default=os.path.join(tempfile.gettempdir(), "cds_eval_out"))
    ap.add_argument("--scan", default="dtu", choices=sorted(SCANS))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    {"tree": cmd_tree, "kernel": cmd_kernel, "host": cmd_host, "pipeline": cmd_pipeline}[args.cmd](args)


if __name__ == "__main__":
    main()
