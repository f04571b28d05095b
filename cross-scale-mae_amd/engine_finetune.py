"""Fine-tuning epoch and evaluation on the MI355X path (reference engine_finetune.py: same signatures, meter names and return dicts).

Differences: the model computes the criterion itself (`model(samples, targets)`; `criterion` keeps its place in the signature and is not
used: main_finetune.py sets `model.smoothing` / the mixup targets instead); `max_norm` 0 or None means no clipping; losses stay on the device and are drained every `args.print_freq` iterations (a non-finite loss raises at
that drain, FusedAdamW skips on the device every update whose loss was not finite); macro / micro F1 come from a numpy confusion matrix
(util.metrics.f1_scores); W&B / TensorBoard logging and the mIoU (`use_psa`) branch are not wired."""
from typing import Iterable, Optional

import numpy as np
import torch

import util.lr_sched as lr_sched
import util.misc as misc
from util.downstream import PendingLosses, autocast
from util.metrics import f1_scores


def train_one_epoch(model: torch.nn.Module, criterion, data_loader: Iterable, optimizer: torch.optim.Optimizer, device: torch.device, epoch: int,
                    loss_scaler, max_norm: float = 0, mixup_fn=None, log_writer=None, args=None, ignore_index=-9999):
    if args is None:
        raise Exception("args is None")
    model.train(True)
    metric_logger = misc.MetricLogger(delimiter="  ")
    metric_logger.add_meter("lr", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    header = f"Epoch: [{epoch}]"
    accum_iter, print_freq = args.accum_iter, getattr(args, "print_freq", 20)
    optimizer.zero_grad()
    n_iters = len(data_loader)
    pending = PendingLosses()   # (with the largest group lr)

    for it, (samples, targets) in enumerate(metric_logger.log_every(data_loader, print_freq, header)):
        if it % accum_iter == 0:   # a per-iteration (not per-epoch) schedule
            lr_sched.adjust_learning_rate(optimizer, it / n_iters + epoch, args)
        samples, targets = samples.to(device, non_blocking=True), targets.to(device, non_blocking=True)
        if mixup_fn is not None:
            samples, targets = mixup_fn(samples, targets)
        with autocast(device):
            loss, _ = model(samples, targets)
        pending.append(loss, max(g["lr"] for g in optimizer.param_groups))
        loss_scaler(loss / accum_iter, optimizer, clip_grad=max_norm or None, parameters=model.parameters(), create_graph=False,
                    update_grad=(it + 1) % accum_iter == 0)
        if (it + 1) % accum_iter == 0:
            optimizer.zero_grad()
        if it % print_freq == 0 or it == n_iters - 1:
            pending.drain(metric_logger)   # exactly the iterations on which log_every prints the meters
    pending.drain(metric_logger)
    metric_logger.synchronize_between_processes()
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


@torch.no_grad()
def evaluate(data_loader, model, device, args=None, ignore_index=-9999):
    """-> {"loss", "acc1", ("acc5" when nb_classes < 4, as the reference), "macro_f1", "micro_f1"}: plain cross-entropy in eval mode."""
    if args is None:
        raise Exception("args is None")
    if getattr(args, "use_psa", False):
        raise NotImplementedError("--use_psa (mIoU evaluation) is not implemented on the MI355X path")
    model.eval()
    model.drain_counts()
    losses, true_labels, predict = [], [], []
    for batch in data_loader:
        images, target = batch[0].to(device, non_blocking=True), batch[-1].to(device, non_blocking=True)
        with autocast(device):
            loss, output = model(images, target)
        losses.append(loss.reshape(()) * images.shape[0])
        true_labels.append(target)
        predict.append(torch.argmax(output, dim=-1))
    top1, top5, seen = model.drain_counts()
    y, pred = torch.cat(true_labels).cpu().numpy().astype(int), torch.cat(predict).cpu().numpy().astype(int)
    macro, micro, classwise = f1_scores(y, pred)
    stats = {"loss": float(torch.stack(losses).sum()) / seen, "acc1": 100.0 * top1 / seen}
    if int(args.nb_classes) < 4:
        stats["acc5"] = 100.0 * top5 / seen
    stats.update(macro_f1=macro, micro_f1=micro)
    print("* Acc@1 {:.3f}\n* CE-loss {:.3f}".format(stats["acc1"], stats["loss"]))
    print(f"* Macro F1 score: {macro:.3f}\n", f"* Micro F1 score: {micro:.3f}\n", f"* Classwise F1 score: {np.asarray(classwise)}")
    return stats
