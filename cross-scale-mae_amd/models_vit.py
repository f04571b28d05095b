"""Plain ViT encoder + classification head for linear probing and fine-tuning (reference models_vit.py: timm's VisionTransformer with optional global
average pooling): the reference's factories, keywords and parameter names, so that `util.checkpoint_keys.to_vit_keys(checkpoint["model"])`
loads with strict=False leaving only `head.*` (and `fc_norm.*` under global pooling) missing.  Every FLOP runs on the MI355X:

* the trunk is the pre-training encoder forward (`csmae_hip.Engine.encode_stream` at mask_ratio 0 with an increasing noise ramp, so the
  token order is the identity): the resident / streaming attention kernels, bf16 MFMA under autocast, exact fp32 otherwise;
* pooling + final norm, the probe's BatchNorm1d, the classifier, cross-entropy with top-1 / top-5 counts run in csrc/classify.hip.

Probe mode (main_linprobe.py:515-525) trains only the head: `loss.backward()` fills `head.1.weight.grad` / `head.1.bias.grad` through one
coarse autograd node.  Fine-tune mode (`finetune_mode()`, main_finetune.py) trains everything: head, final norm and trunk share one flat
buffer, and `loss.backward()` runs the head's backward of csrc/classify.hip and `Engine.backward_stream`.  A model in neither mode refuses
trunk gradients; dropout / drop-path > 0 is not implemented and raises."""
from functools import partial

import torch
import torch.nn as nn

from models_mae._holders import Block, PatchEmbed
from util.checkpoint_keys import from_vit_keys
from util.pos_embed import get_2d_sincos_pos_embed


class _TrunkView:
    """The trunk's Parameters under the pre-training names the engine reads (encoder.<i>.*, encoder_pos_embed, ...), plus the few
    decoder-side slots its constructor looks up (never computed with: the stand-alone encoder half is all that runs)."""

    def __init__(self, vit, P, extra=()):
        own = dict(vit.named_parameters())
        named = from_vit_keys(own)
        named.update((n, own[n]) for n in extra if n in own)   # fine-tune mode: head.* and fc_norm.* live in the same flat buffer, under their own names
        dev = vit.cls_token.device
        stub = lambda *shape: nn.Parameter(torch.zeros(*shape, device=dev), requires_grad=False)
        named.update({"decoder_norm.weight": stub(_STUB_DD), "decoder_norm.bias": stub(_STUB_DD), "decoder_pred.weight": stub(P, _STUB_DD)})
        self._named = list(named.items())

    def named_parameters(self):
        return list(self._named)


_STUB_DD = 8   # width of the decoder slots of the trunk view


class _HeadFn(torch.autograd.Function):
    """One autograd node for trunk + head + loss.  The only differentiable input is a zero-dim anchor (see
    models_mae.MAE_ViT_Baseline._StepFn).  Probe mode: backward = the classifier's weight / bias gradient kernel, written into the `.grad`
    tensors.  Fine-tune mode: classifier dW / db and dX, pooling + final-norm backward into the residual-stream gradient, then the trunk's
    reverse pass (Engine.backward_stream); every gradient lands in the flat buffer, whose views become the `.grad`s.  A backward into
    existing gradients accumulates."""

    @staticmethod
    def forward(ctx, model, x, target, anchor):
        loss, logits, fbn, dlogits = model._pass(x, target, want_grad=True)
        ctx.model, ctx.fbn, ctx.dlogits, ctx.eng = model, fbn, dlogits, None
        if model._finetune:
            ctx.eng = model._engine(x)
            ctx.gen, ctx.loss = ctx.eng.gen, loss.detach()   # (not the output itself: no cycle through its grad_fn)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, gloss, glogits):
        if gloss is not None:
            from csmae_hip import ops
            gscale = gloss.detach().reshape(1).to(torch.float32).contiguous()
            if ctx.eng is not None:
                ctx.model._finetune_backward(ctx.eng, ctx.gen, ctx.fbn, ctx.dlogits, ctx.loss, gscale)
                return (None,) * 4
            lin = ctx.model._linear()
            had = lin.weight.grad is not None or (lin.bias is not None and lin.bias.grad is not None)
            for p in (lin.weight, lin.bias):
                if p is not None and p.grad is None:
                    p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            ops.head_linear_bwd(ctx.dlogits, ctx.fbn, lin.weight.grad, None if lin.bias is None else lin.bias.grad, accumulate=had, gscale=gscale)
        return (None,) * 4


class VisionTransformer(nn.Module):
    """Vision Transformer with support for global average pooling (models_vit.py:17-60)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4,
                 qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), global_pool=False, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.0, **kwargs):
        super().__init__()
        if kwargs:
            raise TypeError(f"unsupported VisionTransformer arguments: {sorted(kwargs)}")
        if drop_rate or attn_drop_rate or drop_path_rate:
            raise NotImplementedError("dropout / drop-path > 0 is not implemented on the MI355X path (main_linprobe.py passes 0)")
        if mlp_ratio != 4 or not qkv_bias:
            raise NotImplementedError("the MI355X blocks are timm's with mlp_ratio 4 and a qkv bias")
        patch_size = int(patch_size)
        assert img_size % patch_size == 0 and embed_dim % num_heads == 0
        if num_classes < 1:
            raise ValueError("num_classes must be positive: the model ends in a classifier")
        self.num_classes, self.embed_dim, self.num_features, self.num_heads = num_classes, embed_dim, embed_dim, num_heads
        self.img_size, self.patch_size, self.in_chans = img_size, patch_size, in_chans
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, norm_layer) for _ in range(depth)])
        self.global_pool = global_pool
        if global_pool:
            self.fc_norm = norm_layer(embed_dim)   # (models_vit.py:32-37: fc_norm replaces norm)
        else:
            self.norm = norm_layer(embed_dim)
        self.head = nn.Linear(embed_dim, num_classes)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        self.apply(self._init_weights)
        # models_vit.py:24-29: the fixed sin-cos table
        table = get_2d_sincos_pos_embed(embed_dim, int(num_patches ** 0.5), cls_token=True)
        self.pos_embed.data.copy_(torch.from_numpy(table).float().unsqueeze(0))
        self.compute_dtype = None  # None: bf16 MFMA under torch autocast, exact fp32 otherwise; or force torch.bfloat16 / torch.float32
        self.smoothing = 0.0       # fine-tune mode, training: label smoothing applied to integer labels (main_finetune.py sets it)
        self._finetune = False
        self._flat, self._view, self._engines, self._bufs = None, None, {}, {}

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    # ---- probe mode (main_linprobe.py:515-525)
    def probe_mode(self):
        """head -> Sequential(BatchNorm1d(affine=False, eps=1e-6), head) with a trunc_normal_(std=2e-5) classifier weight; everything but
        the head is frozen."""
        if not isinstance(self.head, nn.Sequential):
            nn.init.trunc_normal_(self.head.weight, std=2e-5)
            bn = nn.BatchNorm1d(self.head.in_features, affine=False, eps=1e-6).to(self.head.weight.device)
            self.head = nn.Sequential(bn, self.head)
        for p in self.parameters():
            p.requires_grad = False
        for p in self.head.parameters():
            p.requires_grad = True
        return self

    # ---- fine-tune mode (main_finetune.py)
    def finetune_mode(self):
        """Everything trains: `forward(x, target)` returns a loss that is differentiable w.r.t. every parameter.  head.* and the final norm move
        into the trunk's flat buffer at the next forward (one buffer for FusedAdamW, `.grad`s are views of its gradient twin)."""
        if isinstance(self.head, nn.Sequential):
            raise RuntimeError("finetune_mode() on a model in probe mode: the probe head (BatchNorm1d + Linear) is not the fine-tune head")
        for p in self.parameters():
            p.requires_grad = True
        self._finetune = True
        self._flat, self._engines = None, {}   # (re-homed with the head at the next forward)
        return self

    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    def _linear(self):
        return self.head[1] if isinstance(self.head, nn.Sequential) else self.head

    # ---- engine plumbing
    def _cfg(self):
        p, C = self.patch_size, self.in_chans
        G = self.img_size // p
        return dict(S=self.img_size, C=C, p=p, G=G, L=G * G, P=p * p * C, D=self.embed_dim, He=self.num_heads, Ne=len(self.blocks), Dd=_STUB_DD,
                    Hd=1, Nd=0, Hp=0, loss="mse", norm_pix=False, reduction="sum", loss_cd="mse", loss_e="mse", variant="Baseline")

    def _engine(self, x):
        from csmae_hip.engine import Engine, FlatParams
        if not x.is_cuda:
            raise RuntimeError("this model runs only on an MI355X: move the model and the batch to 'cuda' (there is no CPU fallback; "
                               "the CPU restatement lives in oracle/ and is test infrastructure)")
        if not self.cls_token.is_cuda:
            raise RuntimeError("model parameters are on the CPU: call model.to('cuda') first")
        if self._flat is None or not self._flat.still_homed():
            extra = [n for n, _ in self.named_parameters() if n.startswith(("head.", "fc_norm."))] if self._finetune else ()
            self._view = _TrunkView(self, self._cfg()["P"], extra)
            self._flat = FlatParams(self._view, self.cls_token.device)
            self._engines = {}
        dtype = self.compute_dtype
        if dtype is None:
            dtype = torch.bfloat16 if torch.is_autocast_enabled() else torch.float32
        if dtype not in self._engines:
            self._engines[dtype] = Engine(self._view, self._flat, self._cfg(), dtype)
        return self._engines[dtype]

    def _buf(self, name, shape, dtype=torch.float32):
        """A scratch tensor of the model's, re-made when its shape or the device moves."""
        dev = self.cls_token.device
        t = self._bufs.get(name)
        if t is None or t.shape != tuple(shape) or t.device != dev:
            t = self._bufs[name] = torch.empty(shape, device=dev, dtype=dtype)
        return t

    def _check_input(self, x):
        if x.dim() != 4 or x.shape[1] != self.in_chans or x.shape[2] != self.img_size or x.shape[3] != self.img_size:
            raise AssertionError(f"input {tuple(x.shape)} does not match (N, {self.in_chans}, {self.img_size}, {self.img_size})")
        return x.contiguous().float()

    def _stream(self, x, training=False):
        """The residual stream behind the last block, [N, L + 1, D] in the engine's workspace (fp32, or bf16 in throughput mode)."""
        x = self._check_input(x)
        eng = self._engine(x)
        N, L, D = x.shape[0], self.patch_embed.num_patches, self.embed_dim
        ramp = self._bufs.get("ramp")
        if ramp is None or ramp.shape != (N, L) or ramp.device != x.device:   # increasing noise: random_masking's argsort is the identity, nothing is dropped
            ramp = self._bufs["ramp"] = (torch.arange(L, dtype=torch.float32, device=x.device) / L).expand(N, L).contiguous()
        ws = eng.encode_stream(x, 0.0, ramp, training=training)
        return ws.enc["x"][len(self.blocks)].view(N, L + 1, D)

    def _features(self, x, training=False):
        """feat [N, D] fp32 in a buffer of the model's (overwritten by the next call).  `training`: the trunk keeps its activations for one
        Engine.backward_stream."""
        from csmae_hip import ops
        tokens = self._stream(x, training)
        N, D = tokens.shape[0], self.embed_dim
        norm = self.fc_norm if self.global_pool else self.norm
        feat = self._buf("feat", (N, D))
        ops.probe_pool_fwd(tokens, norm.weight.detach(), norm.bias.detach(), feat, self.global_pool, eps=norm.eps)
        return feat

    def _pass(self, x, target, want_grad):
        """Trunk, pooling + final norm, the probe's BatchNorm, classifier, criterion.  `target`: int64 labels [N] (cross-entropy with the top-1 /
        top-5 counters; in fine-tune mode label-smoothed by `self.smoothing` while training) or, in fine-tune mode only, dense float targets
        [N, K] (soft-target cross-entropy); None: logits alone.
        -> loss, logits, the classifier's input (fine-tune mode: the model's feat buffer; else a fresh tensor), dlogits (for a unit upstream
        gradient; None unless want_grad)."""
        from csmae_hip import ops
        ft = self._finetune
        feat = self._features(x, training=ft and want_grad)
        N, D, K, dev = feat.shape[0], self.embed_dim, self.num_classes, feat.device
        lin = self._linear()
        if isinstance(self.head, nn.Sequential):
            bn = self.head[0]
            training = bn.training or bn.running_mean is None
            fbn = torch.empty(N, D, device=dev, dtype=torch.float32)
            ops.bn1d_fwd(feat, fbn, bn.running_mean, bn.running_var, bn.num_batches_tracked, eps=bn.eps, momentum=bn.momentum, training=training)
        else:
            fbn = feat if ft else feat.clone()
        logits = torch.empty(N, K, device=dev, dtype=torch.float32)
        ops.head_linear_fwd(fbn, lin.weight.detach(), None if lin.bias is None else lin.bias.detach(), logits)
        if target is None:
            return None, logits, fbn, None
        hard = target.dtype == torch.int64 and target.shape == (N,)
        if ft:
            if target.device != dev:
                raise ValueError("target must live on the model's device")
            if not hard and not (target.is_floating_point() and target.shape == (N, K)):
                raise ValueError(f"target must be int64 labels of shape ({N},) or dense float targets of shape ({N}, {K})")
        elif not hard or target.device != dev:
            raise ValueError(f"target must be an int64 tensor of shape ({N},) on the model's device")
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        dlogits = torch.empty(N, K, device=dev, dtype=torch.float32) if want_grad else None
        scratch = self._buf("ce_scratch", (3 * N,))
        smoothing = float(self.smoothing) if ft and hard and self.training else 0.0
        if hard and smoothing == 0.0:
            ops.softmax_ce(logits, target.contiguous(), loss, dlogits=dlogits, counts=self.hit_counts(), accumulate_counts=True, scratch=scratch)
            self._seen += N
        else:   # LabelSmoothingCrossEntropy(s) = soft-target cross-entropy on the smoothed one-hot rows
            dense = (ops.mixup_target(target.contiguous(), self._buf("dense_target", (N, K)), lam=1.0, smoothing=smoothing) if hard
                     else target.float().contiguous())
            ops.soft_ce(logits, dense, loss, dlogits=dlogits, scratch=scratch)
        return loss.reshape(()), logits, fbn, dlogits

    def _finetune_backward(self, eng, gen, feat, dlogits, loss, gscale):
        from csmae_hip import ops
        eng.stream_backward_ready(gen)   # (before anything is written: feat and the workspace must still be this forward's)
        flat = self._flat
        G = flat.G
        N, T, D = feat.shape[0], self.patch_embed.num_patches + 1, self.embed_dim
        accumulate = any(p.grad is not None for p in flat.params.values())
        if not accumulate:
            flat.g[: flat.total].zero_()
        ops.gate_accumulate(loss.reshape(1), flat.gate, accumulate)   # FusedAdamW skips the update on the device when a loss behind it was not finite
        ops.head_linear_bwd(dlogits, feat, G("head.weight"), None if self.head.bias is None else G("head.bias"), accumulate=True, gscale=gscale)
        dfeat = self._buf("dfeat", (N, D))
        ops.head_linear_dx(dlogits, self.head.weight.detach(), dfeat, gscale=gscale)
        norm, name = (self.fc_norm, "fc_norm") if self.global_pool else (self.norm, "encoder_norm")
        tokens = eng.ws.enc["x"][len(self.blocks)].view(N, T, D)
        dres = eng.stream_grad().view(N, T, D)
        ops.probe_pool_bwd(tokens, dfeat, norm.weight.detach(), dres, G(name + ".weight"), G(name + ".bias"), self.global_pool, eps=norm.eps,
                           accumulate=True, partial=self._buf("pool_partial", (2 * N * D,)))
        eng.backward_stream(dres, accumulate=True, gen=gen)   # (on top of the head's gradients: the buffer was cleared above)

    # ---- accuracy counters: top-1 / top-5 hits of every `forward(x, target)` since the last drain, kept on the device
    def hit_counts(self):
        c = self.__dict__.get("_counts")
        if c is None or c.device != self.cls_token.device:
            c = self.__dict__["_counts"] = torch.zeros(2, device=self.cls_token.device, dtype=torch.float32)
            self.__dict__["_seen"] = 0
        return c

    def drain_counts(self):
        """-> (top-1 hits, top-5 hits, samples) since the last drain (one host read), and start over."""
        c = self.hit_counts()
        top1, top5 = c.tolist()
        seen, self._seen = self._seen, 0
        c.zero_()
        return top1, top5, seen

    # ---- public API
    @torch.no_grad()
    def forward_features(self, x):
        """[N, D]: pooled (global_pool) or cls-token features behind the final norm (models_vit.py:39-60).  Inference only."""
        return self._features(x).clone()

    @torch.no_grad()
    def forward_patch_tokens(self, x):
        """[N, L, D] fp32: every patch token behind the final norm, the cls token dropped (dense features for main_segprobe.py).  Inference only.
        `global_pool` plays no part: dense features take the model's `norm` (a model built with global_pool=True owns only `fc_norm`, which then
        stands in)."""
        from csmae_hip import ops
        tokens = self._stream(x)
        N, T, D = tokens.shape
        norm = self.norm if hasattr(self, "norm") else self.fc_norm
        out = torch.empty(N * (T - 1), D, device=tokens.device, dtype=torch.float32)
        ops.seg_token_norm(tokens, norm.weight.detach(), norm.bias.detach(), out, eps=norm.eps)
        return out.view(N, T - 1, D)

    def forward(self, x, target=None):
        """logits [N, K]; with `target`: (loss, logits).  Probe mode: int64 class indices, mean cross-entropy, differentiable w.r.t. the head.
        Fine-tune mode: int64 class indices or dense float targets [N, K] (mixup), differentiable w.r.t. every parameter."""
        trainable = [n for n, p in self.named_parameters() if p.requires_grad]
        grad = target is not None and torch.is_grad_enabled() and bool(trainable)
        if grad:
            anchor = self.__dict__.get("_anchor")
            if anchor is None or anchor.device != x.device:
                anchor = self.__dict__["_anchor"] = torch.zeros((), device=x.device, requires_grad=True)
            if not self._finetune and any(not n.startswith("head.") for n in trainable):
                raise NotImplementedError("only the head is trainable on the MI355X path (linear probing): freeze the trunk, e.g. with probe_mode(), or "
                                          f"train all of it with finetune_mode(); got requires_grad on {[n for n in trainable if not n.startswith('head.')][:3]} ...")
            return _HeadFn.apply(self, x, target, anchor)
        with torch.no_grad():
            loss, logits, _, _ = self._pass(x, target, want_grad=False)
        return logits if target is None else (loss, logits)


# the reference's factories (models_vit.py:63-99); a keyword given by the caller wins over the preset (small geometries for tests)
def vit_base_patch16(**kwargs):
    return VisionTransformer(**{**dict(embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6)), **kwargs})


def vit_large_patch16(**kwargs):
    return VisionTransformer(**{**dict(embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6)), **kwargs})


def vit_huge_patch14(**kwargs):
    return VisionTransformer(**{**dict(embed_dim=1280, depth=32, num_heads=16, mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6)), **kwargs})
