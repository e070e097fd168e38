"""Training driver: the reference's four stages behind one CLI.

Reference entry points (each a standalone script there):
  * Part 1  ``/root/reference/src/Part 1/main.py``   single process          -> ``--strategy none``
  * Part 2a ``/root/reference/src/Part 2a/main.py``  gather/scatter sync     -> ``--strategy gather_scatter``
  * Part 2b ``/root/reference/src/Part 2b/main.py``  blocking all-reduce     -> ``--strategy allreduce_blocking``
  * Part 3  ``/root/reference/src/Part 3/main.py``   DDP wrapper             -> ``--strategy ddp``
  plus ``--strategy bucketed_overlap`` (hook-driven bucketed all-reduce on an unwrapped model).

Same flags with the same meaning (``--master``, ``--num-nodes``, ``--rank``, ``--epochs``; port 6585,
global batch 256 split as ``int(256 / W)``), the same seeding, optimizer, loss, train/test loops and
the exact log strings (``Training loss after {} iterations is {}``, ``Forward/Backward/Average Pass
time in iter {} is {}``, ``Test set: Average loss: ...``). Also runs under ``torchrun`` (RANK /
WORLD_SIZE / LOCAL_RANK from the environment).

Deliberate deviation (documented): the reference never calls ``model.train()`` again after the first
``test_model`` (``src/Part 1/main.py:62``), so later epochs train with BatchNorm in eval mode. We
call ``model.train()`` at the start of every epoch; ``--reference-bn-quirk`` restores the original
behaviour.
"""
from __future__ import annotations

import argparse
import os
import time

import torch

from . import distributed as dist
from .data import MIX_MODES, DeviceLoader, DistributedSampler, MixTarget, cifar10_binary, synthetic_cifar10, synthetic_imagenet
from .models import get_model
from .ops import BinaryCrossEntropy, CrossEntropyLoss, count_correct
from .optim import LAMB, LARS, SGD, AdamW, LRSchedule
from .parallel import (
    BucketedOverlap,
    DistributedDataParallel,
    average_gradients_allreduce,
    average_gradients_gather_scatter,
)
from .utils import PhaseTimer, latest_checkpoint, load_checkpoint, save_checkpoint, seed_everything
from .utils import profiling
from .utils.profiling import TraceRecorder


def _phase(trace, name):
    """A traced phase (chrome trace + roctx) or just a roctx range (emitted when CDP_ROCTX=1)."""
    return trace.phase(name) if trace is not None else profiling.range(name)


def train_model(model, train_loader, optimizer, criterion, rank=0, sync=None, strategy="none", max_iters=None,
                timer=None, on_iter=None, trace=None, print_fn=print):
    """One epoch. ``sync`` is the reference's ``average_gradients`` hook (or a BucketedOverlap)."""
    iter_number = 1
    epoch_loss = 0
    timer = timer or PhaseTimer(None)
    # Part 1/2a/2b print "epochs", Part 3 "iterations" (src/Part 1/main.py:49, src/Part 2a/main.py:104,
    # src/Part 2b/main.py:104, src/Part 3/main.py:105)
    unit = "iterations" if strategy in ("ddp", "bucketed_overlap") else "epochs"
    for batch_idx, (data, target) in enumerate(train_loader):
        timer.mark("start")
        with _phase(trace, "forward"):
            optimizer.zero_grad()
            predictions = model(data)
            if isinstance(sync, BucketedOverlap):
                sync.prepare(predictions)
        timer.mark("forward")
        with _phase(trace, "backward"):
            loss = criterion(predictions, target)
            loss.backward()
        if strategy in ("gather_scatter", "allreduce_blocking"):
            with _phase(trace, "sync"):
                if strategy == "gather_scatter":
                    average_gradients_gather_scatter(model, rank)
                else:
                    average_gradients_allreduce(model)
        with _phase(trace, "step"):
            optimizer.step()
        timer.mark("backward")

        epoch_loss += loss.detach()
        if on_iter is not None:
            on_iter(iter_number, loss)
        if iter_number % 20 == 0:
            epoch_loss = epoch_loss / 20
            print_fn("Training loss after {} {} is {}".format(iter_number, unit, epoch_loss))
            epoch_loss = 0
            fwd = timer.pop("forward")
            bwd = timer.pop("backward")
            if iter_number != 20:
                print_fn("Forward Pass time in iter {} is {}".format(iter_number, fwd / 20.0))
                print_fn("Backward Pass time in iter {} is {}".format(iter_number, bwd / 20.0))
                print_fn("Average Pass time in iter {} is {}".format(iter_number, (fwd + bwd) / 20.0))
            if getattr(optimizer, "grad_norm", None) is not None:
                # gradient clipping on: the window's last norm (stderr: stdout keeps the reference's lines)
                import sys

                print("[cdp] rank {}: grad norm in iter {} is {} (clip coef {}, skipped steps {})".format(
                    rank, iter_number, float(optimizer.grad_norm), float(optimizer.clip_coef),
                    int(optimizer.skipped_steps)), file=sys.stderr)
            if getattr(optimizer, "trust_ratios", None) is not None:
                # LARS: the spread of the window's last trust ratios (stderr, as the clip line)
                import sys

                tr = optimizer.trust_ratios
                print("[cdp] rank {}: trust ratio in iter {} is min {} max {}".format(
                    rank, iter_number, float(tr.min()), float(tr.max())), file=sys.stderr)
            if getattr(optimizer, "last_lr", None) is not None:
                # learning-rate schedule: the rate of the window's last step, and the step index the next
                # one will use (stderr, as above)
                import sys

                print("[cdp] rank {}: lr in iter {} is {} (schedule step {})".format(
                    rank, iter_number, float(optimizer.last_lr), int(optimizer.schedule_step)), file=sys.stderr)
            if isinstance(target, MixTarget):
                # mixup / CutMix: the window's last mix, as the loader's kernel published it (stderr, as above)
                import sys

                info = target.info.tolist()
                print("[cdp] rank {}: mix in iter {} is mode {} lam {}".format(
                    rank, iter_number, MIX_MODES[int(info[0])], info[1]), file=sys.stderr)
            crops = getattr(train_loader, "last_crops", None)
            if crops is not None and not (data.is_cuda and torch.cuda.is_current_stream_capturing()):
                # RandomResizedCrop: the first image's window in the window's last batch (stderr, as above)
                import sys

                top, left, h, w = crops[0, :4].tolist()
                print("[cdp] rank {}: crop of image 0 in iter {} is {} x {} at ({}, {})".format(
                    rank, iter_number, h, w, top, left), file=sys.stderr)
            erase = getattr(train_loader, "last_erase", None)
            if erase is not None and not (data.is_cuda and torch.cuda.is_current_stream_capturing()):
                # RandomErasing: the first image's box in the window's last batch (stderr, as above)
                import sys

                on, top, left, h, w = erase[0].tolist()
                print("[cdp] rank {}: erase of image 0 in iter {} is {}".format(
                    rank, iter_number, "{} x {} at ({}, {})".format(h, w, top, left) if on else "none"),
                    file=sys.stderr)
            ra_rows = getattr(train_loader, "last_randaug", None)
            if ra_rows is not None and not (data.is_cuda and torch.cuda.is_current_stream_capturing()):
                # RandAugment: the first image's operations in the window's last batch (stderr, as above)
                import sys

                from .randaug import describe

                print("[cdp] rank {}: randaug of image 0 in iter {} is {}".format(
                    rank, iter_number, " ".join(describe(r) for r in ra_rows[0].tolist())), file=sys.stderr)
            scales = getattr(getattr(model, "module", model), "last_drop_scales", None)
            if scales is not None and not (data.is_cuda and torch.cuda.is_current_stream_capturing()):
                # stochastic depth: the branches the window's last forward dropped (stderr, as above)
                import sys

                print("[cdp] rank {}: drop path in iter {} dropped {} of {} branches".format(
                    rank, iter_number, int((scales == 0).sum()), scales.numel()), file=sys.stderr)
        if max_iters is not None and iter_number >= max_iters:
            break
        iter_number += 1
    return iter_number


def test_model(model, test_loader, criterion, print_fn=print, topk=None):
    """The reference's eval loop; ``topk`` (``--eval-topk K``) also counts top-K hits in a second device
    counter and prints them to stderr (stdout keeps the reference's line)."""
    model.eval()
    test_loss = 0
    correct = None
    correct_k = None
    n = 0
    with torch.no_grad():
        for batch_idx, (data, target) in enumerate(test_loader):
            output = model(data)
            test_loss += criterion(output, target)
            correct = count_correct(output, target, correct)
            if topk is not None:
                correct_k = count_correct(output, target, correct_k, topk=topk)
            n += 1
    test_loss /= max(1, n)
    correct = int(correct.sum().item()) if correct is not None else 0
    total = len(test_loader.dataset)
    print_fn(
        "Test set: Average loss: {:.4f}, Accuracy: {}/{} ({:.0f}%)\n".format(
            float(test_loss), correct, total, 100.0 * correct / total
        )
    )
    if topk is not None:
        import sys

        ck = int(correct_k.sum().item()) if correct_k is not None else 0
        print("[cdp] top-{} accuracy: {}/{} ({:.0f}%)".format(topk, ck, total, 100.0 * ck / total), file=sys.stderr)
    return float(test_loss), correct


def build_data(args, device, train: bool):
    if args.data.startswith("cifar10-bin:"):
        return cifar10_binary(args.data.split(":", 1)[1], train=train, device=device)
    if args.model.startswith("resnet"):
        n = args.synthetic_size or (1281 if train else 500)
        return synthetic_imagenet(n, seed=0 if train else 1, device=device, size=args.stored_size)
    n = args.synthetic_size or (50000 if train else 10000)
    return synthetic_cifar10(n, seed=0, device=device, train=train, learnable=args.data == "synthetic-learnable")


def run(rank, size, epochs, batch_size, args):
    seed_everything(args.seed)
    batch_size = int(batch_size / float(dist.get_world_size()))
    device = dist.device() if dist.is_initialized() else args.device_obj
    training_set = build_data(args, device, True)
    train_sampler = DistributedSampler(training_set, num_replicas=size, rank=rank) if size > 1 else None
    # mixup / CutMix shape the training batches only: the test loader below takes none of it
    train_loader = DeviceLoader(training_set, batch_size, sampler=train_sampler, shuffle=(size == 1), train=True,
                                seed=args.seed, mixup_alpha=args.mixup_alpha, cutmix_alpha=args.cutmix_alpha,
                                mix_prob=args.mix_prob, mix_switch_prob=args.mix_switch_prob,
                                out_size=args.crop_size if args.rrc_scale is not None else None,
                                rrc_scale=args.rrc_scale, rrc_ratio=args.rrc_ratio, erase_prob=args.random_erase,
                                erase_scale=args.erase_scale, erase_ratio=args.erase_ratio,
                                erase_mode=args.erase_mode, randaug_num_ops=args.randaug[0],
                                randaug_magnitude=args.randaug[1], randaug_mstd=args.randaug_mstd,
                                randaug_ops=args.randaug_ops, randaug_fill=args.randaug_fill)
    print("Size of training set is {}".format(len(train_loader)))
    test_set = build_data(args, device, False)
    test_loader = DeviceLoader(test_set, batch_size, shuffle=False, train=False, out_size=args.crop_size,
                               center_crop=args.center_crop)
    print("Size of test set is {}".format(len(test_loader)))

    if dist.is_initialized() and device.type == "cuda":
        # which communicator carries the gradient collectives (stderr: stdout keeps the reference's lines)
        import sys

        kind = "rccl-native" if dist.native_communicator() is not None else "torch-" + str(dist.get_backend())
        print(f"[cdp] rank {rank}: collectives on {kind}"
              + (f" ({dist.comm_fallback_reason()})" if dist.comm_fallback_reason() else ""), file=sys.stderr)
    # label smoothing shapes the training loss only: the eval loss stays the plain cross-entropy
    # (--loss bce: every logit a one-vs-rest sigmoid classifier, against the same smoothed / mixed targets)
    if getattr(args, "loss", "ce") == "bce":
        criterion = BinaryCrossEntropy(label_smoothing=args.label_smoothing, target_threshold=args.bce_target_thresh,
                                       sum_classes=args.bce_sum_classes)
    else:
        criterion = CrossEntropyLoss(label_smoothing=args.label_smoothing)
    eval_criterion = CrossEntropyLoss()
    model_kw = {}
    if args.model.startswith("resnet"):
        # stochastic depth and the zero-initialised last BatchNorm live in the model; every rank draws its own
        # masks (its seed is derived from --seed and the rank)
        model_kw = dict(drop_path_rate=args.drop_path, drop_path_seed=args.seed * 1000003 + rank,
                        zero_init_residual=args.zero_init_residual)
    model = get_model(args.model, **model_kw).to(device)
    sync = None
    strategy = args.strategy
    if strategy == "ddp":
        model = DistributedDataParallel(model, bucket_cap_mb=args.bucket_cap_mb)
    elif strategy == "bucketed_overlap":
        sync = BucketedOverlap(model, bucket_cap_mb=args.bucket_cap_mb)
    lr_schedule = _lr_schedule_from(args, epochs, len(train_loader))
    # --weight-decay: the reference's 1e-4 for sgd / lars, the conventional 0.01 for adamw / lamb
    wd = args.weight_decay
    if wd is None:
        wd = 0.01 if args.optimizer in ("adamw", "lamb") else 0.0001
    common = dict(max_grad_norm=args.clip_grad_norm, skip_nonfinite=args.skip_nonfinite, ema_decay=args.ema_decay,
                  lr_schedule=lr_schedule)
    if args.optimizer in ("adamw", "lamb"):
        cls = AdamW if args.optimizer == "adamw" else LAMB
        kw = {} if args.adam_eps is None else {"eps": args.adam_eps}  # else the class's own default
        optimizer = cls(model.parameters(), lr=args.lr, betas=tuple(args.betas), weight_decay=wd, **kw, **common)
    elif args.optimizer == "lars":
        optimizer = LARS(model.parameters(), lr=args.lr, momentum=0.9, weight_decay=wd,
                         trust_coefficient=args.trust_coefficient, max_grad_norm=args.clip_grad_norm,
                         skip_nonfinite=args.skip_nonfinite, ema_decay=args.ema_decay, lr_schedule=lr_schedule)
    else:
        optimizer = SGD(model.parameters(), lr=args.lr, momentum=0.9, weight_decay=wd,
                        max_grad_norm=args.clip_grad_norm, skip_nonfinite=args.skip_nonfinite,
                        ema_decay=args.ema_decay, lr_schedule=lr_schedule)

    start_epoch = 0
    if args.resume and args.checkpoint_dir:
        path = _agreed_checkpoint(args.checkpoint_dir, size)
        if path:
            st = load_checkpoint(path, model, optimizer, map_location=device)
            start_epoch = st.get("epoch", 0)
            print("Resumed from {} (epoch {})".format(path, start_epoch))
    trace = TraceRecorder(rank, device) if args.trace else None
    reducer = _reducer_of(model, sync)
    if trace is not None and reducer is not None:
        reducer.set_trace(True)
    for epoch in range(start_epoch, epochs):
        if not args.reference_bn_quirk or epoch == 0:
            model.train()
        start_time = time.time()
        timer = PhaseTimer(device)
        train_model(model, train_loader, optimizer, criterion, rank, sync=sync, strategy=strategy,
                    max_iters=args.iters, timer=timer, trace=trace)
        if device.type == "cuda":
            torch.cuda.synchronize()
        print("Training time after {} epoch is {}".format(epoch + 1, (time.time() - start_time)))
        test_model(model, test_loader, eval_criterion, topk=args.eval_topk)
        if args.ema_decay is not None:
            # once more with the averaged weights (stderr: stdout keeps the reference's lines); BatchNorm
            # evaluates with the live running statistics
            import sys

            with optimizer.ema_weights():
                ema_loss, ema_correct = test_model(model, test_loader, eval_criterion, print_fn=lambda *_: None)
            total = len(test_loader.dataset)
            print("[cdp] EMA weights: Average loss: {:.4f}, Accuracy: {}/{} ({:.0f}%)".format(
                ema_loss, ema_correct, total, 100.0 * ema_correct / total), file=sys.stderr)
        if args.checkpoint_dir:
            save_checkpoint(os.path.join(args.checkpoint_dir, f"ckpt_{epoch + 1}.pt"), model, optimizer,
                            epoch=epoch + 1, rank=rank)
    if trace is not None:
        if reducer is not None:
            trace.add_reducer_log(reducer.trace_log())
        path = args.trace if size == 1 else "{}.rank{}{}".format(*os.path.splitext(args.trace)[:1], rank,
                                                                 os.path.splitext(args.trace)[1] or ".json")
        trace.dump(path)
    return model


def _lr_schedule_from(args, epochs, loader_len):
    """The ``--lr-schedule`` flags as an :class:`LRSchedule` over the whole run (None without them):
    ``total_steps = epochs * iterations per epoch``, milestones given in epochs. ``--warmup-iters``
    alone means a constant schedule behind the warm-up. ``--resume`` continues it from the checkpoint's
    step (the optimizer's ``state_dict`` carries it)."""
    kind = args.lr_schedule
    if kind is None:
        if not args.warmup_iters:
            return None
        kind = "constant"
    per_epoch = min(loader_len, args.iters) if args.iters is not None else loader_len
    return LRSchedule(kind, total_steps=epochs * per_epoch, warmup_steps=args.warmup_iters,
                      warmup_start_factor=args.warmup_start_factor, end_factor=args.lr_end_factor,
                      power=args.poly_power, milestones=[e * per_epoch for e in args.lr_milestones],
                      gamma=args.lr_gamma)


def _reducer_of(model, sync):
    if isinstance(model, DistributedDataParallel):
        return model.reducer
    if isinstance(sync, BucketedOverlap):
        return sync.reducer
    return None


def _agreed_checkpoint(directory, size):
    """Rank 0 picks the checkpoint; every rank must be able to read that same file.

    Only rank 0 writes checkpoints, so without a shared filesystem other ranks would silently start
    from scratch while rank 0 resumes (diverged replicas, mismatched epoch counts, hung collectives).
    """
    path = latest_checkpoint(directory) if dist.get_rank() == 0 else None
    if size == 1 or not dist.is_initialized():
        return path
    import torch.distributed as tdist

    box = [path]
    tdist.broadcast_object_list(box, src=0)
    path = box[0]
    if path is None:
        return None
    ok = torch.tensor([1 if os.path.isfile(path) else 0], dtype=torch.int64,
                      device=dist.device() if dist.device().type == "cuda" else "cpu")
    tdist.all_reduce(ok, op=tdist.ReduceOp.MIN)
    if int(ok.item()) != 1:
        raise RuntimeError(f"--resume: checkpoint {path} (chosen by rank 0) is not readable on every rank; "
                           "use a shared --checkpoint-dir")
    return path


def init_process(master, port, rank, size, fn, epochs=1, batch_size=256, backend="rccl", args=None):
    """Initialize the distributed environment (``src/Part 2a/main.py:148-153``)."""
    os.environ["MASTER_ADDR"] = master
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group(backend, rank=rank, world_size=size)
    try:
        return fn(rank, size, epochs, batch_size, args)
    finally:
        dist.destroy_process_group()


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Process arguments for training")
    p.add_argument("--master", metavar="master-address", default=os.environ.get("MASTER_ADDR"),
                   help="The IP address of Master")
    p.add_argument("--num-nodes", metavar="total-nodes", type=int, default=None, help="Total number of nodes")
    p.add_argument("--rank", metavar="rank", type=int, default=None, help="Rank of this node")
    p.add_argument("--epochs", metavar="epochs", type=int, default=1, help="Number of epochs")
    p.add_argument("--port", default=os.environ.get("MASTER_PORT", "6585"))
    p.add_argument("--backend", default=None, choices=["rccl", "nccl", "gloo"])
    p.add_argument("--strategy", default=None,
                   choices=["none", "gather_scatter", "allreduce_blocking", "bucketed_overlap", "ddp"])
    p.add_argument("--model", default="vgg11")
    p.add_argument("--data", default="synthetic",
                   help="synthetic (random labels) | synthetic-learnable (labels a fixed function of the image) "
                        "| cifar10-bin:<root>")
    p.add_argument("--synthetic-size", type=int, default=None)
    p.add_argument("--batch-size", type=int, default=256, help="global batch (split int(B/W) per rank)")
    p.add_argument("--lr", type=float, default=0.1)
    p.add_argument("--iters", type=int, default=None, help="max iterations per epoch")
    p.add_argument("--lr-schedule", default=None, choices=["constant", "cosine", "poly", "step"],
                   help="scale --lr by a schedule evaluated inside the fused optimizer step, over epochs x iterations "
                        "per epoch steps (default: none, every step at --lr)")
    p.add_argument("--warmup-iters", type=int, default=0, metavar="N",
                   help="linear warm-up over the first N steps (alone: a constant schedule behind it)")
    p.add_argument("--warmup-start-factor", type=float, default=0.0, metavar="F",
                   help="the warm-up starts at F x --lr")
    p.add_argument("--lr-end-factor", type=float, default=0.0, metavar="F",
                   help="cosine / poly end at F x --lr")
    p.add_argument("--poly-power", type=float, default=2.0, metavar="P",
                   help="power of --lr-schedule poly (1: linear decay, 2: the LARS paper's)")
    p.add_argument("--lr-milestones", type=int, nargs="+", default=[], metavar="E",
                   help="epochs at which --lr-schedule step multiplies the rate by --lr-gamma")
    p.add_argument("--lr-gamma", type=float, default=0.1, metavar="G", help="factor of --lr-schedule step")
    p.add_argument("--optimizer", default="sgd", choices=["sgd", "lars", "adamw", "lamb"],
                   help="sgd (the reference's), lars: SGD with layer-wise adaptive rate scaling, for large batches, "
                        "adamw, or lamb: AdamW's update with a layer-wise trust ratio (set --lr to suit: 1e-3 is usual)")
    p.add_argument("--betas", type=float, nargs=2, default=(0.9, 0.999), metavar=("B1", "B2"),
                   help="decay rates of the two moments (--optimizer adamw / lamb)")
    p.add_argument("--adam-eps", type=float, default=None, metavar="FLOAT",
                   help="eps of --optimizer adamw (default 1e-8) / lamb (default 1e-6)")
    p.add_argument("--weight-decay", type=float, default=None, metavar="FLOAT",
                   help="weight decay (default: 1e-4 for sgd / lars, 0.01 for adamw / lamb)")
    p.add_argument("--trust-coefficient", type=float, default=0.001, metavar="FLOAT",
                   help="LARS trust coefficient (--optimizer lars)")
    p.add_argument("--clip-grad-norm", type=float, default=None, metavar="FLOAT",
                   help="clip the global gradient 2-norm to this value inside the fused optimizer step")
    p.add_argument("--skip-nonfinite", action="store_true",
                   help="skip an optimizer step whose gradients hold an inf or a NaN")
    p.add_argument("--ema-decay", type=float, default=None, metavar="FLOAT",
                   help="keep an exponential moving average of the weights inside the fused optimizer step and "
                        "evaluate it too after every epoch (stderr); checkpoints carry it")
    p.add_argument("--label-smoothing", type=float, default=0.0, metavar="FLOAT",
                   help="train against (1 - FLOAT) * onehot + FLOAT / classes (the test loss stays unsmoothed)")
    p.add_argument("--loss", default="ce", choices=["ce", "bce"],
                   help="training loss: softmax cross-entropy (ce, the reference's) or binary cross-entropy with logits "
                        "over the same index / mixed targets (bce); --label-smoothing feeds either, the test loss "
                        "stays the plain cross-entropy")
    p.add_argument("--bce-target-thresh", type=float, default=None, metavar="FLOAT",
                   help="--loss bce: binarise the smoothed / mixed target, 1 where it is above FLOAT in [0, 1)")
    p.add_argument("--bce-sum-classes", action="store_true",
                   help="--loss bce: sum the loss over the classes and average over the batch (default: mean over both)")
    p.add_argument("--mixup-alpha", type=float, default=0.0, metavar="FLOAT",
                   help="mixup: blend every training batch with its reverse, lam ~ Beta(FLOAT, FLOAT) per batch (0: off)")
    p.add_argument("--cutmix-alpha", type=float, default=0.0, metavar="FLOAT",
                   help="CutMix: paste a box of the reversed batch, its area from Beta(FLOAT, FLOAT) (0: off)")
    p.add_argument("--mix-prob", type=float, default=1.0, metavar="FLOAT",
                   help="probability that a training batch is mixed at all (with --mixup-alpha / --cutmix-alpha)")
    p.add_argument("--mix-switch-prob", type=float, default=0.5, metavar="FLOAT",
                   help="probability of CutMix over mixup when both alphas are set")
    p.add_argument("--rrc-scale", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="RandomResizedCrop on the training loader: a window of U(LO, HI) of the image area, resized "
                        "to --crop-size (replaces the pad-shift RandomCrop)")
    p.add_argument("--rrc-ratio", type=float, nargs=2, default=(3.0 / 4.0, 4.0 / 3.0), metavar=("LO", "HI"),
                   help="aspect ratio range of the RandomResizedCrop window (log-uniform)")
    p.add_argument("--random-erase", type=float, default=0.0, metavar="PROB",
                   help="RandomErasing of the training images: one box per image with probability PROB, after crop / "
                        "resize / flip / normalise and before mixup / CutMix (0: off)")
    p.add_argument("--erase-mode", choices=("const", "rand", "pixel"), default="const",
                   help="the erased box's fill: zeros (const), one N(0, 1) value per channel (rand) or per element (pixel)")
    p.add_argument("--erase-scale", type=float, nargs=2, default=(0.02, 0.33), metavar=("LO", "HI"),
                   help="the erased box's share of the image area")
    p.add_argument("--erase-ratio", type=float, nargs=2, default=(0.3, 3.3), metavar=("LO", "HI"),
                   help="the erased box's aspect ratio h / w (log-uniform)")
    p.add_argument("--randaug", type=float, nargs=2, default=(0, 9.0), metavar=("N", "M"),
                   help="RandAugment of the training images: N operations per image at magnitude M in [0, 30], on the "
                        "uint8 image after crop / resize / flip and before the normalisation (N = 0: off)")
    p.add_argument("--randaug-mstd", type=float, default=0.0, metavar="S",
                   help="RandAugment: standard deviation of the per-operation magnitude noise (timm's mstd)")
    p.add_argument("--randaug-ops", nargs="+", default=None, metavar="NAME",
                   help="RandAugment: the operations to draw from (default: all 14)")
    p.add_argument("--randaug-fill", type=int, nargs=3, default=None, metavar=("R", "G", "B"),
                   help="RandAugment: the geometric operations' value outside the image (default: 255 * mean)")
    p.add_argument("--drop-path", type=float, default=0.0, metavar="FLOAT",
                   help="stochastic depth of the resnet models: the last residual block drops its branch per image "
                        "with probability FLOAT, block i of L with FLOAT * i / (L - 1) (0: off)")
    p.add_argument("--zero-init-residual", action="store_true",
                   help="resnet models: start every block's last BatchNorm weight at 0")
    p.add_argument("--crop-size", type=int, default=None, metavar="S",
                   help="output side of both loaders (training: with --rrc-scale; default: the stored size)")
    p.add_argument("--center-crop", type=float, default=None, metavar="FRAC",
                   help="test loader: the central FRAC of each side, resized to --crop-size")
    p.add_argument("--stored-size", type=int, default=224, metavar="S",
                   help="side of the synthetic ImageNet-shaped images (resnet models)")
    p.add_argument("--eval-topk", type=int, default=None, metavar="K",
                   help="also report the top-K accuracy of the test set (stderr; ties go to the lower class index)")
    p.add_argument("--bucket-cap-mb", type=float, default=None)
    p.add_argument("--device", default="auto", choices=["auto", "cpu", "cuda"])
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--checkpoint-dir", default=None)
    p.add_argument("--resume", action="store_true")
    p.add_argument("--trace", default=None,
                   help="write a chrome trace (phases + reducer hook/bucket-launch events) to this path "
                        "(.rankN suffix per rank when distributed)")
    p.add_argument("--num-threads", type=int, default=4,
                   help="CPU intra-op threads for the CPU path (the reference pins 4: src/Part 1/main.py:11)")
    p.add_argument("--reference-bn-quirk", action="store_true",
                   help="reproduce the reference's missing model.train() after the first eval")
    args = p.parse_args(argv)
    if args.loss != "bce" and (args.bce_target_thresh is not None or args.bce_sum_classes):
        p.error("--bce-target-thresh and --bce-sum-classes need --loss bce")
    if args.bce_target_thresh is not None and not 0.0 <= args.bce_target_thresh < 1.0:
        p.error("--bce-target-thresh must be in [0, 1)")
    if not args.model.lower().startswith("resnet") and (args.drop_path != 0.0 or args.zero_init_residual):
        p.error("--drop-path and --zero-init-residual apply to the resnet models only")
    if not 0.0 <= args.drop_path < 1.0:
        p.error("--drop-path must be in [0, 1)")
    if args.randaug[0] != int(args.randaug[0]):
        p.error("--randaug N M: N is a whole number of operations")
    args.randaug = (int(args.randaug[0]), float(args.randaug[1]))
    if args.randaug_fill is not None:
        args.randaug_fill = tuple(args.randaug_fill)
    return args


def main(argv=None):
    args = parse_args(argv)
    size = args.num_nodes if args.num_nodes is not None else int(os.environ.get("WORLD_SIZE", "1"))
    rank = args.rank if args.rank is not None else int(os.environ.get("RANK", "0"))
    if args.device == "auto":
        args.device_obj = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    else:
        args.device_obj = torch.device(args.device)
    if args.device_obj.type == "cpu":
        torch.set_num_threads(args.num_threads)
    if args.strategy is None:
        args.strategy = "ddp" if size > 1 else "none"
    if size > 1 or args.strategy != "none":
        backend = args.backend or ("rccl" if args.device_obj.type == "cuda" else "gloo")
        master = args.master or "127.0.0.1"
        return init_process(master, args.port, rank, size, run, args.epochs, args.batch_size, backend, args)
    return run(0, 1, args.epochs, args.batch_size, args)


if __name__ == "__main__":
    main()
