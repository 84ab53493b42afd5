"""Train or fine-tune from DTU / BlendedMVS scenes on disk: the reference's ``Trainer._train_epoch`` (trainer/trainer.py:38-100) and
``BaseTrainer.train`` / ``_save_checkpoint`` / ``_resume_checkpoint`` (base/base_trainer.py:57-169) around ``train.train_step``.

    python -m cds_mvsnet_amd.fit --dataset blended --datapath <BlendedMVS> --trainlist <list> --vallist <list> \
        --num_srcs 3 --interval_scale 1.0 --batch_size 2 --epochs 10 --save_dir saved/ [--pretrained ckpt.pth | --resume ckpt.pth] [--graph]

Epochs are 1-based.  For each epoch: the DynamicConv temperature of ``train.temperature_for_epoch``; every training set in turn, every
batch of ``train_data.TrainBatches`` through ``train_step`` (``--graph``: ``train.CapturedTrainStep``); one scheduler step; every
``eval_freq`` epochs and on epoch ``epochs - 1`` (trainer.py:96) ``depth_eval.validate`` at temperature 0.01 over each validation set
(``mode="val"``, 5 views, no shuffle).  The loss is read on the host only every ``logging_every`` steps (the reference reads it every
step, which stalls the host behind the GPU); the epoch means are summed on the device and read once.  Checkpoints carry the
reference's five keys with a plain-dict ``config`` and load through ``infer.load_checkpoint`` without ``trust_pickle``.

Differences from the reference, on purpose: its ``_train_epoch`` returns the training means only, so ``monitor`` never finds a
validation metric and switches itself off; here the validation scalars (of the last validation set, as its meter would hold them) are
part of the epoch's record and ``--monitor "min abs_depth_error"`` works.  There is no early stop and no TensorBoard.  The reference
saves no optimiser state (SGD without momentum has none); ``--resume`` restores the weights, starts at ``epoch + 1`` and advances the
scheduler to match.  Under ``torchrun`` the gradients are averaged with ``train.GradAllReducer`` and every rank reads its own shard of
the batches; that path is wired but has not been run on more than one GPU.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
from typing import Dict, List, Optional, Sequence

import torch

from . import depth_eval, train_data
from . import train as T

VAL_VIEWS = 5
VAL_TEMPERATURE = 0.01                                        # trainer.py:98
CHECKPOINT_KEYS = ("arch", "epoch", "state_dict", "monitor_best", "config")
DATASETS = {"dtu": train_data.DTUTrainScenes, "blended": train_data.BlendedTrainScenes}


def save_checkpoint(path: str, model: torch.nn.Module, epoch: int, monitor_best: float, config: Optional[dict] = None) -> None:
    """base_trainer.py:118-140: {'arch', 'epoch', 'state_dict', 'monitor_best', 'config'}; ``config`` must be a plain dict of builtins (the
    reference pickles its ConfigParser, which ``weights_only=True`` refuses), so the file loads with ``infer.load_checkpoint``."""
    config = {} if config is None else config
    json.dumps(config)                                        # raises on anything that is not plain data
    state = {"arch": type(model).__name__, "epoch": int(epoch),
             "state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
             "monitor_best": float(monitor_best), "config": config}
    tmp = path + ".tmp"
    torch.save(state, tmp)
    os.replace(tmp, path)


def parse_monitor(monitor: Optional[str]):
    """'off' / None -> (None, None); 'min abs_depth_error' -> ('min', 'abs_depth_error') (base_trainer.py:29-36)."""
    if monitor is None or monitor == "off":
        return None, None
    parts = monitor.split()
    if len(parts) != 2 or parts[0] not in ("min", "max"):
        raise ValueError(f"monitor {monitor!r}: expected 'off' or '<min|max> <metric>'")
    return parts[0], parts[1]


def _dist_rank_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def fit(model: torch.nn.Module, train_sets: Sequence, val_sets: Sequence, epochs: int, batch_size: int = 2, val_batch_size: int = 1,
        lr: float = 1e-4, weight_decay: float = 0.01, step_size: int = 3, gamma: float = 0.5,
        dlossw: Sequence[float] = (0.5, 1.0, 2.0), eval_freq: int = 1, save_period: int = 1, save_dir: Optional[str] = None,
        logging_every: int = 100, monitor: Optional[str] = "off", resume: Optional[str] = None, graph: bool = False,
        conv_arithmetic: Optional[str] = None, activation_storage: Optional[str] = None, threads: int = 4, ahead: int = 2,
        config: Optional[dict] = None, log=print) -> List[Dict[str, object]]:
    """Train ``model`` (on its ROCm device) for epochs ``start .. epochs`` over ``train_sets`` (``train_data`` datasets in train mode),
    validating on ``val_sets`` (datasets in val mode).  -> the per-epoch records, also written to ``<save_dir>/log.json``:
    {"epoch", "temperature", "lr", "steps", "loss", "depth_loss" (means over the epoch's steps), "logged": [[step, loss, depth_loss], ...]
    for the steps whose loss was read, "val": {loss, depth_loss, the twelve metrics} when validation ran}."""
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("fit trains on the GPU only: move the model to a ROCm (cuda) device")
    mode, metric = parse_monitor(monitor)
    best = math.inf if mode != "max" else -math.inf
    start = 1
    if resume is not None:
        from .infer import load_checkpoint
        load_checkpoint(model, resume)
        ck = torch.load(resume, map_location="cpu", weights_only=True)
        start = int(ck["epoch"]) + 1
        best = float(ck.get("monitor_best", best))
    rank, world = _dist_rank_world()
    reducer = T.GradAllReducer(model.parameters(), module=model) if world > 1 else None
    optimizer = T.make_optimizer(model, lr=lr, weight_decay=weight_decay)
    scheduler = T.make_scheduler(optimizer, step_size=step_size, gamma=gamma)
    for _ in range(1, start):                                 # the epochs the checkpoint has behind it
        optimizer.step()                                      # no gradients yet: a no-op that keeps StepLR's call-order check quiet
        scheduler.step()
    step = T.CapturedTrainStep(model, optimizer, reducer=reducer, dlossw=dlossw, activation_storage=activation_storage,
                               conv_arithmetic=conv_arithmetic) if graph else None
    if save_dir is not None and rank == 0:
        os.makedirs(save_dir, exist_ok=True)
    logging_every = max(1, int(logging_every))
    records: List[Dict[str, object]] = []
    for epoch in range(start, int(epochs) + 1):
        temperature = T.temperature_for_epoch(epoch)
        lr_now = float(optimizer.param_groups[0]["lr"])
        log("Epoch {} temperature {}".format(epoch, temperature))
        model.train()
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        steps, logged = 0, []
        for ds in train_sets:
            with train_data.TrainBatches(ds, batch_size, dev, epoch=epoch, rank=rank, world=world, threads=threads, ahead=ahead) as dl:
                for batch_idx, sample in enumerate(dl):
                    t0 = time.time()
                    if step is not None:
                        loss, depth_loss = step(sample, temperature)
                    else:
                        loss, depth_loss = T._step_tensors(model, optimizer, sample, temperature, dlossw, reducer, activation_storage,
                                                           conv_arithmetic=conv_arithmetic)
                    sums += torch.stack((loss, depth_loss)).double()
                    steps += 1
                    if batch_idx % logging_every == 0:        # the only host read of the step
                        lv, dv = float(loss), float(depth_loss)
                        logged.append([steps - 1, lv, dv])
                        log("Epoch {}/{}, Iter {}/{}, lr {:.6f}, train loss = {:.3f}, depth loss = {:.3f}, time = {:.3f}".format(
                            epoch, epochs, batch_idx, len(dl), lr_now, lv, dv, time.time() - t0))
        scheduler.step()
        means = (sums / max(steps, 1)).cpu().tolist()
        rec: Dict[str, object] = {"epoch": epoch, "temperature": temperature, "lr": lr_now, "steps": steps, "loss": means[0],
                                  "depth_loss": means[1], "logged": logged}
        if val_sets and (epoch % max(1, int(eval_freq)) == 0 or epoch == int(epochs) - 1):
            for ds in val_sets:
                with train_data.TrainBatches(ds, val_batch_size, dev, epoch=epoch, shuffle=False, drop_last=False, rank=rank, world=world,
                                             threads=threads, ahead=ahead) as dl:
                    rec["val"] = depth_eval.validate(model, dl, VAL_TEMPERATURE, dlossw)
                log("{} avg_test_scalars: {}".format(ds.datapath, rec["val"]))
        for key in ("epoch", "loss", "depth_loss"):
            log("    {:15s}: {}".format(key, rec[key]))
        improved = False
        if mode is not None and "val" in rec:
            if metric not in rec["val"]:
                raise KeyError(f"monitor metric {metric!r} is not among the validation scalars {sorted(rec['val'])}")
            v = float(rec["val"][metric])
            improved = (mode == "min" and v <= best) or (mode == "max" and v >= best)
            if improved:
                best = v
        rec["best"] = improved
        records.append(rec)
        if save_dir is not None and rank == 0:
            if epoch % max(1, int(save_period)) == 0:
                path = os.path.join(save_dir, "checkpoint-epoch{}.pth".format(epoch))
                save_checkpoint(path, model, epoch, best, config)
                log("Saving checkpoint: {} ...".format(path))
            if improved:
                save_checkpoint(os.path.join(save_dir, "model_best.pth"), model, epoch, best, config)
                log("Saving current best: model_best.pth ...")
            with open(os.path.join(save_dir, "log.json"), "w") as f:
                json.dump(records, f, indent=1)
    return records


# ---------------------------------------------------------------------------------------------------------------------
# command line: the fields of configs/config_*.json
def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m cds_mvsnet_amd.fit",
                                 description="train / fine-tune CDS-MVSNet on DTU or BlendedMVS scenes on disk, on the GPU")
    ap.add_argument("--dataset", action="append", choices=sorted(DATASETS), required=True,
                    help="repeat for several training sets (config_all_dataset), each with its --datapath / --trainlist / --vallist")
    ap.add_argument("--datapath", action="append", required=True)
    ap.add_argument("--trainlist", action="append", required=True)
    ap.add_argument("--vallist", action="append", default=[])
    ap.add_argument("--num_srcs", type=int, default=3, help="views per training sample INCLUDING the reference view (the reference's "
                                                            "loaders pass num_srcs as nviews)")
    ap.add_argument("--num_depths", type=int, default=192)
    ap.add_argument("--interval_scale", type=float, default=1.06)
    ap.add_argument("--crop", default=None, metavar="H,W",
                    help="centre crop of images and ground truth, for every dataset (default: the layout's own, 512,640 for dtu and "
                         "576,768 for blended); a tree of render --export_blended needs the size of its maps or less")
    ap.add_argument("--batch_size", type=int, default=2)
    ap.add_argument("--val_batch_size", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--weight_decay", type=float, default=0.01)
    ap.add_argument("--step_size", type=int, default=3)
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--dlossw", default="0.5,1.0,2.0")
    ap.add_argument("--eval_freq", type=int, default=1)
    ap.add_argument("--save_period", type=int, default=1)
    ap.add_argument("--save_dir", default="saved")
    ap.add_argument("--logging_every", type=int, default=100)
    ap.add_argument("--monitor", default="off", help="'off' or e.g. 'min abs_depth_error': keep model_best.pth")
    ap.add_argument("--pretrained", default=None, help="start from these weights at epoch 1")
    ap.add_argument("--resume", default=None, help="continue a run: weights, epoch + 1, scheduler")
    ap.add_argument("--trust-checkpoint", dest="trust_checkpoint", action="store_true",
                    help="--pretrained is one of the reference's own files (pickled ConfigParser): read it through the restricted unpickler")
    ap.add_argument("--graph", action="store_true", help="replay the step as a captured hipGraph (train.CapturedTrainStep)")
    ap.add_argument("--conv_arithmetic", default=None, choices=["f32", "split_f16"])
    ap.add_argument("--activation_storage", default=None, choices=["f32", "bf16"])
    ap.add_argument("--threads", type=int, default=4, help="decode threads (1..16)")
    ap.add_argument("--ahead", type=int, default=2, help="batches decoded ahead; 0 = synchronous")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    n = len(args.dataset)
    if len(args.datapath) != n or len(args.trainlist) != n or len(args.vallist) not in (0, n):
        ap.error("give --datapath and --trainlist once per --dataset, and --vallist for all of them or none")
    if args.pretrained and args.resume:
        ap.error("--pretrained and --resume exclude each other")
    try:
        args.dlossw = [float(x) for x in args.dlossw.split(",")]
        if args.crop is not None:
            args.crop = [int(x) for x in args.crop.split(",")]
            if len(args.crop) != 2 or min(args.crop) < 1:
                raise ValueError(f"--crop {args.crop}: expected H,W, both positive")
        parse_monitor(args.monitor)
    except ValueError as e:
        ap.error(str(e))
    return args


def main(argv: Optional[Sequence[str]] = None) -> List[Dict[str, object]]:
    from . import CDSMVSNet, seeded_init_
    from .infer import load_checkpoint
    args = parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)
    arch = {"refine": True, "ndepths": [48, 32, 8], "depth_interals_ratio": [4.0, 2.0, 1.0]}      # configs/config_*.json "arch"
    model = CDSMVSNet(refine=True, ndepths=tuple(arch["ndepths"]), depth_interals_ratio=tuple(arch["depth_interals_ratio"]))
    if args.pretrained:
        load_checkpoint(model, args.pretrained, trust_pickle=args.trust_checkpoint)
    elif not args.resume:
        seeded_init_(model, args.seed)
    model = model.to(dev)
    train_sets, val_sets = [], []
    for i, name in enumerate(args.dataset):
        train_sets.append(DATASETS[name](args.datapath[i], args.trainlist[i], "train", args.num_srcs, args.num_depths, args.interval_scale,
                                         crop=args.crop, seed=args.seed))
        if args.vallist:
            val_sets.append(DATASETS[name](args.datapath[i], args.vallist[i], "val", VAL_VIEWS, args.num_depths, args.interval_scale,
                                           crop=args.crop, seed=args.seed))
    config = {"arch": {"type": "CDSMVSNet", "args": arch}, "args": {k: v for k, v in vars(args).items()}}
    try:
        return fit(model, train_sets, val_sets, args.epochs, batch_size=args.batch_size, val_batch_size=args.val_batch_size, lr=args.lr,
                   weight_decay=args.weight_decay, step_size=args.step_size, gamma=args.gamma, dlossw=args.dlossw, eval_freq=args.eval_freq,
                   save_period=args.save_period, save_dir=args.save_dir, logging_every=args.logging_every, monitor=args.monitor,
                   resume=args.resume, graph=args.graph, conv_arithmetic=args.conv_arithmetic, activation_storage=args.activation_storage,
                   threads=args.threads, ahead=args.ahead, config=config)
    finally:
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
