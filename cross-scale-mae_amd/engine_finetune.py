"""Fine-tuning epoch and evaluation on the MI355X path (reference engine_finetune.py: same signatures, meter names and return dicts).

Differences: the model computes the criterion itself (`model(samples, targets)`; `criterion` keeps its place in the signature and is not
used: main_finetune.py sets `model.smoothing` / the mixup targets instead); `max_norm` 0 or None means no clipping; losses stay on the device and are drained every `args.print_freq` iterations (a non-finite loss raises at
that drain, FusedAdamW skips on the device every update whose loss was not finite); macro / micro F1 come from a numpy confusion matrix
(util.metrics.f1_scores); W&B / TensorBoard logging and the mIoU (`use_psa`) branch are not wired."""
from typing import Iterable, Optional

import numpy as np
import torch

from util.downstream import autocast, train_epoch
from util.metrics import f1_scores


def train_one_epoch(model: torch.nn.Module, criterion, data_loader: Iterable, optimizer: torch.optim.Optimizer, device: torch.device, epoch: int,
                    loss_scaler, max_norm: float = 0, mixup_fn=None, log_writer=None, args=None, ignore_index=-9999):
    if args is None:
        raise Exception("args is None")
    accum_iter = args.accum_iter

    def update(loss, it):   # the loss scaler runs backward, and clips and steps at the end of each accumulation window
        last = (it + 1) % accum_iter == 0
        loss_scaler(loss / accum_iter, optimizer, clip_grad=max_norm or None, parameters=model.parameters(), create_graph=False, update_grad=last)
        if last:
            optimizer.zero_grad()
    optimizer.zero_grad()
    return train_epoch(model, data_loader, optimizer, device, epoch, args, update, transform=mixup_fn)


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
