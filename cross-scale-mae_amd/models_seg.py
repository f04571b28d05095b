"""Linear segmentation probe of a frozen ViT encoder (main_segprobe.py): the dense counterpart of the linear classification probe of
models_vit.py.  The trunk is `VisionTransformer.forward_patch_tokens` (the stand-alone encoder + the final LayerNorm on every patch token,
inference only); the head is BatchNorm1d(D, affine=False) + Linear(D, K) over the N L patch rows, built from the classification probe's kernels
(csrc/classify.hip); the criterion upsamples the [N, G, G, K] patch logits bilinearly to the label resolution inside the loss kernel
(csrc/segment.hip: the upsampled logits never reach memory) and scores them against uint8 labels with an ignore value.  Every FLOP runs on
the MI355X; `loss.backward()` fills the head's `.grad` tensors through one coarse autograd node."""
import torch
import torch.nn as nn


class _SegFn(torch.autograd.Function):
    """One autograd node for trunk + head + loss, as models_vit._HeadFn: the only differentiable input is a zero-dim anchor; backward = the
    classifier's weight / bias gradient kernel over the N L patch rows, written into (or accumulated onto) the `.grad` tensors."""

    @staticmethod
    def forward(ctx, probe, x, labels, anchor):
        loss, pl, fbn, dpl = probe._pass(x, labels, want_grad=True)
        ctx.probe, ctx.fbn, ctx.dpl = probe, fbn, dpl
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(pl)
        return loss, pl

    @staticmethod
    def backward(ctx, gloss, gpl):
        if gloss is not None:
            from csmae_hip import ops
            lin = ctx.probe.linear
            gscale = gloss.detach().reshape(1).to(torch.float32).contiguous()
            had = lin.weight.grad is not None or lin.bias.grad is not None
            for p in (lin.weight, lin.bias):
                if p.grad is None:
                    p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            K = lin.out_features
            ops.head_linear_bwd(ctx.dpl.view(-1, K), ctx.fbn, lin.weight.grad, lin.bias.grad, accumulate=had, gscale=gscale)
        return (None,) * 4


class LinearSegProbe(nn.Module):
    """`vit` (a models_vit.VisionTransformer, put into probe mode and frozen as a whole — its own classification head is not used) under a
    per-patch linear classifier.  Labels: uint8 [N, S, S] class indices with S the model's image size, `ignore_index` (255, the only value the
    kernels know) for pixels that take no part; values in [num_classes, 255) are the caller's to keep out — the kernels do not detect them.
    2 <= num_classes <= 64; patch size 4, 8, 14 or 16."""

    def __init__(self, vit, num_classes, ignore_index=255):
        super().__init__()
        from csmae_hip import SEG_IGNORE
        if ignore_index != SEG_IGNORE:
            raise NotImplementedError(f"ignore_index {ignore_index}: the MI355X kernels leave out label {SEG_IGNORE} only (remap the masks)")
        if not 2 <= int(num_classes) <= 64:
            raise ValueError(f"num_classes = {num_classes}: the segmentation kernels hold 2 .. 64 classes")
        self.vit = vit.probe_mode()
        for p in self.vit.parameters():
            p.requires_grad = False
        self.num_classes, self.ignore_index = int(num_classes), ignore_index
        D = vit.embed_dim
        self.bn = nn.BatchNorm1d(D, affine=False, eps=1e-6)
        self.linear = nn.Linear(D, self.num_classes)
        nn.init.trunc_normal_(self.linear.weight, std=0.01)
        nn.init.constant_(self.linear.bias, 0)
        self.to(vit.cls_token.device)
        self._bufs = {}

    def train(self, mode=True):
        super().train(mode)
        self.vit.eval()   # (the trunk is frozen: nothing in it has a training mode)
        return self

    def head_parameters(self):
        return list(self.linear.parameters())

    def _check_labels(self, x, labels):
        N, S = x.shape[0], self.vit.img_size
        if labels.dtype != torch.uint8 or labels.shape != (N, S, S) or labels.device != x.device:
            raise ValueError(f"labels must be a uint8 tensor of shape ({N}, {S}, {S}) on the model's device, got {labels.dtype} {tuple(labels.shape)}")
        return labels.contiguous()

    def _scratch(self, dev):
        from csmae_hip import ops
        t = self._bufs.get("scratch")
        if t is None or t.device != dev:
            t = self._bufs["scratch"] = torch.empty(ops.SEG_CE_SCRATCH_FLOATS, device=dev, dtype=torch.float32)
        return t

    def _logits(self, x):
        """-> patch logits [N, G, G, K] and the classifier's input [N L, D] (fresh tensors)"""
        from csmae_hip import ops
        tok = self.vit.forward_patch_tokens(x)
        N, L, D = tok.shape
        G = self.vit.img_size // self.vit.patch_size
        feat = tok.view(N * L, D)
        bn = self.bn
        fbn = torch.empty_like(feat)
        ops.bn1d_fwd(feat, fbn, bn.running_mean, bn.running_var, bn.num_batches_tracked, eps=bn.eps, momentum=bn.momentum, training=bn.training)
        pl = torch.empty(N * L, self.num_classes, device=feat.device, dtype=torch.float32)
        ops.head_linear_fwd(fbn, self.linear.weight.detach(), self.linear.bias.detach(), pl)
        return pl.view(N, G, G, self.num_classes), fbn

    def _pass(self, x, labels, want_grad, conf=None):
        """-> loss (zero-dim), patch logits, the classifier's input, dpl (for a unit upstream gradient; None unless want_grad)"""
        from csmae_hip import ops
        labels = self._check_labels(x, labels)
        pl, fbn = self._logits(x)
        loss = torch.empty(1, device=pl.device, dtype=torch.float32)
        count = torch.empty(1, device=pl.device, dtype=torch.int64)
        dpl = torch.empty_like(pl) if want_grad else None
        ops.seg_ce(pl, labels, loss, count, dpl=dpl, conf=conf, scratch=self._scratch(pl.device))
        self.last_count = count
        return loss.reshape(()), pl, fbn, dpl

    def forward(self, x, labels=None):
        """Without labels: the argmax class of every pixel, uint8 [N, S, S].  With labels: (loss, patch_logits [N, G, G, K]) — the mean
        cross-entropy over the pixels whose label is not `ignore_index` (0 when there is none; torch would give NaN), differentiable w.r.t. the
        head (BatchNorm has no parameters; its running statistics move in training mode)."""
        from csmae_hip import ops
        if labels is None:
            with torch.no_grad():
                pl, _ = self._logits(x)
                N, S = pl.shape[0], self.vit.img_size
                pred = torch.empty(N, S, S, device=pl.device, dtype=torch.uint8)
                ops.seg_ce(pl, None, torch.empty(1, device=pl.device), torch.empty(1, device=pl.device, dtype=torch.int64), pred=pred,
                           scratch=self._scratch(pl.device))
            return pred
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.linear.parameters()):
            anchor = self.__dict__.get("_anchor")
            if anchor is None or anchor.device != x.device:
                anchor = self.__dict__["_anchor"] = torch.zeros((), device=x.device, requires_grad=True)
            return _SegFn.apply(self, x, labels, anchor)
        with torch.no_grad():
            loss, pl, _, _ = self._pass(x, labels, want_grad=False)
        return loss, pl

    @torch.no_grad()
    def evaluate_batch(self, x, labels, conf, want_logits=False):
        """Adds the batch's confusion counts (rows = true class, columns = predicted class; ignored pixels skipped) into conf [K, K] int64 on the
        device and returns (loss, valid-pixel count [1] int64), both on the device; with want_logits also, as a third value, the patch logits
        [N, G, G, K] of this very forward (what csmae_segpanel draws and counts from).  Call in eval mode: the running statistics normalise."""
        loss, pl, _, _ = self._pass(x, labels, want_grad=False, conf=conf)
        if want_logits:
            return loss, self.last_count, pl
        return loss, self.last_count
