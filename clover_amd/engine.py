"""Data-parallel training engine for the Clover pre-training step on MI355X.

What the reference spreads over MMDistributedDataParallel (tools/train.py:146-154), mmcv's
DefaultOptimizerConstructor + AdamW (pretrain_webvid_cc3m.py:129-137), Fp16OptimizerHook
(mmcv_Fp16OptimizerHook.py:96-149) and the CosineAnnealing LR hook (:139-140) is one object:

* one process per GPU; parameters, gradients and Adam moments live in FLAT fp32 buffers
  (decay / no-decay segments), so the gradient exchange is a handful of large RCCL
  all-reduces over xGMI instead of per-tensor traffic, launched from autograd hooks as soon
  as a bucket is complete (overlapping the rest of backward), and exactly once per step —
  the reference all-reduces twice (DDP reducer + allreduce_grads);
* gradient averaging (the 1/W that gives the reference's R6 behaviour), global-norm clipping
  (max_norm 15) and AdamW run as two HIP kernels per segment (clv_sumsq, clv_adamw_step) with
  no host synchronisation — the reference syncs the host once per parameter for its overflow
  check (fp16_utils.py:328-349); bf16 needs no loss scaling, non-finite norms skip the step;
* statically unused parameters (BERT pooler, the fusion model's own embeddings — the reason
  the reference needs find_unused_parameters=True) are detected on a dry run and excluded;
* ``virtual_ranks=k``: one optimizer step on k micro-batches whose contrastive losses see all k * B rows — what a k-rank
  DDP job of the reference computes, on one device (``CloverEngine.forward_backward``);
* ``ema_enable`` / ``ema_update`` / ``ema_swap``: the reference's ``ema_hook`` (mmaction/core/hooks/ema.py) — an fp32 moving
  average of the weights in a slab of its own per segment, updated and exchanged with the weights by one HIP launch each.
"""
import contextlib
import inspect
import math

import os

import torch
import torch.distributed as dist

from .utils.dist import collectives_active
import torch.nn as nn

from . import ops
from .utils.grad_reducer import BucketedGradReducer


def paramwise_weight_decay(model, base_wd, norm_decay_mult=0.0, bias_decay_mult=0.0, custom_keys=None):
    """mmcv DefaultOptimizerConstructor rules: custom_keys by substring
    (longest first) > norm layers > bias > default.  Returns {param_name: weight_decay}."""
    custom_keys = custom_keys or {}
    sorted_keys = sorted(sorted(custom_keys.keys()), key=len, reverse=True)
    norm_types = (nn.modules.batchnorm._BatchNorm, nn.modules.instancenorm._InstanceNorm, nn.GroupNorm, nn.LayerNorm)
    out = {}
    for mod_name, mod in model.named_modules():
        for pname, p in mod.named_parameters(recurse=False):
            full = f'{mod_name}.{pname}' if mod_name else pname
            wd = base_wd
            hit = False
            for key in sorted_keys:
                if key in full:
                    wd = base_wd * custom_keys[key].get('decay_mult', 1.0)
                    hit = True
                    break
            if not hit:
                if isinstance(mod, norm_types):
                    wd = base_wd * norm_decay_mult
                elif pname == 'bias':
                    wd = base_wd * bias_decay_mult
            out[full] = wd
    return out


def paramwise_options(model, base_wd, paramwise_cfg=None):
    """mmcv 1.3.x DefaultOptimizerConstructor.add_params, per parameter:
    {name: (weight_decay, lr_mult)}.  A ``custom_keys`` hit (substring, longest key first) decides both
    ``lr_mult`` and ``decay_mult`` and switches the other rules off; otherwise ``bias_lr_mult`` applies to every
    ``bias`` outside norm layers, and the decay is ``norm_decay_mult`` for norm layers, else ``bias_decay_mult`` for
    a ``bias``, else 1."""
    cfg = paramwise_cfg or {}
    custom_keys = cfg.get('custom_keys') or {}
    sorted_keys = sorted(sorted(custom_keys.keys()), key=len, reverse=True)
    norm_types = (nn.modules.batchnorm._BatchNorm, nn.modules.instancenorm._InstanceNorm, nn.GroupNorm, nn.LayerNorm)
    out = {}
    for mod_name, mod in model.named_modules():
        is_norm = isinstance(mod, norm_types)
        for pname, p in mod.named_parameters(recurse=False):
            full = f'{mod_name}.{pname}' if mod_name else pname
            wd, lr_mult = base_wd, 1.0
            for key in sorted_keys:
                if key in full:
                    lr_mult = custom_keys[key].get('lr_mult', 1.0)
                    wd = base_wd * custom_keys[key].get('decay_mult', 1.0)
                    break
            else:
                if pname == 'bias' and not is_norm:
                    lr_mult = cfg.get('bias_lr_mult', 1.0)
                if is_norm:
                    wd = base_wd * cfg.get('norm_decay_mult', 1.0)
                elif pname == 'bias':
                    wd = base_wd * cfg.get('bias_decay_mult', 1.0)
            out[full] = (float(wd), float(lr_mult))
    return out


def cosine_lr(base_lr, it, max_iters, min_lr_ratio=1e-3, warmup_iters=0, warmup_ratio=1e-3):
    """mmcv CosineAnnealing (by_epoch=False) with linear warm-up."""
    end = base_lr * min_lr_ratio
    lr = end + 0.5 * (base_lr - end) * (1 + math.cos(math.pi * min(it, max_iters) / max(1, max_iters)))
    if it < warmup_iters:
        k = (1 - it / warmup_iters) * (1 - warmup_ratio)
        lr = lr * (1 - k)
    return lr


class _Segment:
    """A flat fp32 slab: params / grads / exp_avg / exp_avg_sq of one (weight_decay, lr_mult) class — what mmcv
    expresses as one param group per parameter collapses to one slab per DISTINCT option pair."""

    def __init__(self, named_params, weight_decay, device, lr_mult=1.0):
        self.weight_decay = weight_decay
        self.lr_mult = lr_mult
        self.names = [n for n, _ in named_params]
        self.params = [p for _, p in named_params]
        # 16-byte aligned slots (fp32 AND bf16 views: the GEMM kernels take 16-byte aligned operands).  A parameter may ask for PHANTOM rows behind its last one (``_clv_pad_rows``: the MLM
        # decoder's [30522, H] weight and [30522] bias -> 30528, a multiple of 64): the padded [rows + pad, ...] views of the
        # fp32 data, the gradient and the bf16 shadow are what its GEMMs run on (16-byte row groups, no edge code); the
        # phantom rows start at zero, receive zero gradients (the loss kernel zeroes the padding columns of d logits) and
        # so stay zero under AdamW; the module-visible parameter is the unpadded view.
        def slot_elems(p):
            pad = int(getattr(p, '_clv_pad_rows', 0) or 0)
            return p.numel() + pad * (p.numel() // p.shape[0] if p.dim() > 0 and p.shape[0] > 0 else 0)
        sizes = [(slot_elems(p) + 7) // 8 * 8 for p in self.params]          # 8 elements: the bf16 shadow slots are 16-byte aligned too
        self.offsets = [0]
        for s in sizes:
            self.offsets.append(self.offsets[-1] + s)
        n = self.offsets[-1]
        self.flat_p = torch.zeros(n, device=device, dtype=torch.float32)
        self.flat_g = torch.zeros(n, device=device, dtype=torch.float32)
        self.exp_avg = torch.zeros(n, device=device, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros(n, device=device, dtype=torch.float32)
        self.shadow = torch.zeros(n, device=device, dtype=ops.BF16)      # 16-bit compute copy (bf16, or fp16 with CLOVER_HALF=f16)
        for p, off in zip(self.params, self.offsets):
            view = self.flat_p[off:off + p.numel()].view_as(p)
            view.copy_(p.data)
            p.data = view
            hook = getattr(p, '_clv_unscale', None)        # (the recognizer's loss-scale hook of a plain-autograd parameter:
            if hook is not None:                           # under the engine every gradient in the slab stays scaled)
                hook.remove()
                p._clv_unscale = None
            p.grad = self.flat_g[off:off + p.numel()].view_as(p)
            p._clv_grad = p.grad                                                   # sink for ops.linear
            p._clv_shadow = self.shadow[off:off + p.numel()].view_as(p)
            pad = int(getattr(p, '_clv_pad_rows', 0) or 0)
            if pad:
                shp = (p.shape[0] + pad,) + tuple(p.shape[1:])
                n = slot_elems(p)
                p._clv_pad_weight = self.flat_p[off:off + n].view(shp)
                p._clv_pad_grad = self.flat_g[off:off + n].view(shp)
                p._clv_pad_shadow = self.shadow[off:off + n].view(shp)
        self.shadow.copy_(self.flat_p)
        self.shadow_t, self._t_table = None, None
        self._fused = []                     # fused views handed out (fused_view), for build_transposed()

    def build_transposed(self):
        """bf16 W^T copies for the Linear weights whose input-gradient GEMM is a K-contiguous HIP kernel
        (ops.linear_dgrad): one batched transpose per optimizer step refreshes them all.  A fused view (BERT Q|K|V,
        applied as ONE [3H, H] GEMM) gets the transpose of the fused matrix, [H, 3H]; its members then need none of
        their own.  Called once, after the engine has made the fused views."""
        fused_members = {id(m) for f in self._fused if getattr(f, '_clv_want_t', False) for m in f._clv_members}
        def tshape(p):                       # a phantom-padded weight is transposed with its phantom rows
            pad = int(getattr(p, '_clv_pad_rows', 0) or 0)
            return (p.shape[0] + pad, p.shape[1])
        want = [(p, off, tshape(p)) for p, off in zip(self.params, self.offsets)
                if getattr(p, '_clv_want_t', False) and p.dim() == 2 and id(p) not in fused_members]
        want += [(f, f._clv_off, tuple(f.shape)) for f in self._fused if getattr(f, '_clv_want_t', False) and f.dim() == 2]
        if not want or not self.flat_p.is_cuda:
            return
        device = self.flat_p.device
        self.shadow_t = torch.zeros(sum((sh[0] * sh[1] + 7) // 8 * 8 for _, _, sh in want), device=device, dtype=ops.BF16)
        entries, toff = [], 0
        for p, off, shape in want:
            n = shape[0] * shape[1]
            entries.append((off, toff, shape[0], shape[1]))
            view = self.shadow_t[toff:toff + n].view(shape[1], shape[0])
            if shape[0] != p.shape[0]:
                p._clv_pad_shadow_t = view         # [cols, rows + pad]: only the padded kernels may take it
            else:
                p._clv_shadow_t = view
            toff += (n + 7) // 8 * 8
        self._t_table = ops.transpose_table(entries, device)
        self.refresh_transposed()

    def refresh_transposed(self):
        if self._t_table is not None:
            tab, n, tiles = self._t_table
            ops.transpose_batch(self.shadow, self.shadow_t, tab, n, tiles)

    def fused_view(self, members):
        """One Parameter-like view over `members` (adjacent slots of this slab, equal trailing dims,
        concatenated along dim 0): fp32 data, bf16 shadow and gradient sink are slices of the slabs, so a
        module that applies the members as ONE GEMM (BERT Q|K|V) needs no cat / cast / gradient split."""
        idx = [next(i for i, q in enumerate(self.params) if q is m) for m in members]
        assert idx == list(range(idx[0], idx[0] + len(idx))), 'fusion group is not adjacent in the slab'
        assert all(m.numel() % 8 == 0 and m.shape[1:] == members[0].shape[1:] for m in members)      # slots are 8-element aligned
        off, n = self.offsets[idx[0]], sum(m.numel() for m in members)
        shape = (sum(m.shape[0] for m in members),) + tuple(members[0].shape[1:])
        f = torch.nn.Parameter(self.flat_p[off:off + n].view(shape))
        f._clv_grad = self.flat_g[off:off + n].view(shape)
        f._clv_shadow = self.shadow[off:off + n].view(shape)
        f._clv_members = list(members)
        f._clv_ready = lambda ms=f._clv_members: [m._clv_ready() for m in ms] and None
        f._clv_off = off
        f._clv_want_t = all(getattr(m, '_clv_want_t', False) for m in members)
        self._fused.append(f)
        return f


def _complement(spans, total):
    """The ranges of [0, total) that the sorted (begin, end) ``spans`` leave out, in order and none of them empty; spans
    may touch or overlap.  Spans and ranges together tile [0, total)."""
    ranges, pos = [], 0
    for a, b in spans:
        if a > pos:
            ranges.append((pos, a))
        pos = max(pos, b)
    if pos < total:
        ranges.append((pos, total))
    return ranges


class _Capture:
    """The captured step of ONE batch geometry: its hipGraphs and the static tensors they read and write.  capture()
    builds it as a local object and publishes it whole (``engine._captures[sig]``, then ``_activate``); everything of
    the active geometry but the assignable ``engine.graph`` is reached through ``engine._active``."""
    __slots__ = ('graph', 'graph_bwd', 'graph_bwd_video', 'graph_bwd_text', 'graph_loss', 'loss_io', 'batch', 'emb',
                 'mlm', 'demb', 'dmlm', 'cuts', 'stale_views', 'prepacked')

    def __init__(self, graph, graph_bwd, graph_bwd_video, graph_bwd_text, batch, emb, mlm, demb, dmlm, cuts,
                 stale_views, prepacked):
        self.graph, self.graph_bwd = graph, graph_bwd          # encode, and its backward from d emb / d mlm down
        self.graph_bwd_video = graph_bwd_video                 # data-parallel: the video encoder's cut graphs, else None
        self.graph_bwd_text = graph_bwd_text                   # ... and the text encoder's, or None
        self.graph_loss, self.loss_io = None, None             # the loss section as a graph (_capture_loss_graph), or None
        self.batch = batch                                     # static inputs
        self.emb, self.mlm, self.demb, self.dmlm = emb, mlm, demb, dmlm
        self.cuts = cuts                                       # the cut leaves (kept alive with the graphs)
        self.stale_views = stale_views                         # first-touch slots this geometry's backward never writes
        self.prepacked = prepacked                             # buckets whose wire copy the backward graphs write


# Methods through which the step graph enters a module WITHOUT nn.Module.__call__ (the pending-residual form of the Swin
# blocks and patch mergings, the patch embedding's token layouts, the projection head's two towers): torch's forward hooks do
# not see those calls, so the activation report wraps them on the watched instances.
ACT_ENTRY_METHODS = ('forward_pending', 'tokens', 'tokens_stacked', 'forward_text', 'forward_vision')


def default_watched_modules(model):
    """The block-level modules the activation report watches unless told otherwise, as named_modules() names: the patch
    embedding, every Swin block, every patch merging and the Swin final norm; the embeddings module and every transformer
    layer of the text and the fusion encoder; the fusion encoder's input projection (``fc_in`` where the widths differ, and
    the ``norm`` that closes the projection); every head that is a direct child of the recognizer."""
    from .backbones.bert_layers import BertEmbeddings, BertLayer
    from .backbones.cross_transformer import CrossModalTransformerFromPretrained
    from .backbones.swin_transformer_3d import PatchEmbed3D, PatchMerging, SwinTransformer3D, SwinTransformerBlock3D
    names = []
    for name, mod in model.named_modules():
        if isinstance(mod, (PatchEmbed3D, SwinTransformerBlock3D, PatchMerging, BertEmbeddings, BertLayer)):
            names.append(name)
        elif isinstance(mod, SwinTransformer3D):
            names.append(f'{name}.norm')
        elif isinstance(mod, CrossModalTransformerFromPretrained):
            names += [f'{name}.{c}' for c in ('fc_in', 'norm') if hasattr(mod, c)]
    heads_pkg = __name__.rsplit('.', 1)[0] + '.heads'
    names += [name for name, child in model.named_children() if type(child).__module__.startswith(heads_pkg)]
    return names


class _ActivationWatch:
    """The host side of the activation report (csrc/act_report.hip): one 16-byte device record per watched module, folded
    into by one clv_act_report launch per floating tensor of the module's output — inside the step's hipGraphs, because
    the hooks fire while the graphs are captured.  ``on`` gates every launch: the engine sets it only around the forward
    passes it drives itself, so an evaluation or any other caller of the model leaves the table alone."""

    def __init__(self, model, spec, device):
        import fnmatch
        modules = dict(model.named_modules())
        wanted = set(n for n in default_watched_modules(model) if n in modules)
        patterns = list(spec.get('modules') or []) if isinstance(spec, dict) else []
        self._asked = {}                       # pattern -> the modules it added
        for pat in patterns:
            hit = [n for n in modules if n and fnmatch.fnmatchcase(n, pat)]
            if not hit:
                raise ValueError(f'activation_report: the pattern {pat!r} matches no module of {type(model).__name__}')
            wanted.update(hit)
            self._asked[pat] = hit
        self.watched = [n for n in modules if n in wanted]      # registration order, until the dry run has given the forward order
        self.names, self.slot, self.numel = [], {}, {}          # forward order: slot i belongs to names[i]
        self.live, self.latched = ops.act_report_new(len(self.watched), device)
        self.on, self.discover, self.stale = False, True, True
        self._depth = {}
        self._fired, self._clock = {}, 0
        self._undo = []
        for name in self.watched:
            self._install(name, modules[name])

    def _install(self, name, mod):
        def enter(*_a, **_k):
            self._depth[name] = self._depth.get(name, 0) + 1

        def leave(output):
            d = self._depth[name] = self._depth.get(name, 1) - 1
            if d == 0 and self.on:
                self.scan(name, output)

        self._undo.append(mod.register_forward_pre_hook(enter).remove)
        self._undo.append(mod.register_forward_hook(lambda _m, _i, output: leave(output)).remove)
        for meth in ACT_ENTRY_METHODS:
            inner = getattr(mod, meth, None)
            if inner is None or not callable(inner):
                continue

            def entry(*a, _inner=inner, **k):
                enter()
                try:
                    output = _inner(*a, **k)
                except BaseException:
                    self._depth[name] -= 1
                    raise
                leave(output)
                return output
            object.__setattr__(mod, meth, entry)
            self._undo.append(lambda _mod=mod, _meth=meth: object.__delattr__(_mod, _meth))

    def remove(self):
        for undo in self._undo:
            undo()
        self._undo = []

    @staticmethod
    def tensors(output):
        """Every floating HIP tensor of a module's output: a tensor, or tuples / lists / dicts of them."""
        if torch.is_tensor(output):
            return [output] if output.is_cuda and output.is_floating_point() else []
        if isinstance(output, dict):
            return [t for o in output.values() for t in _ActivationWatch.tensors(o)]
        if isinstance(output, (tuple, list)):
            return [t for o in output for t in _ActivationWatch.tensors(o)]
        return []

    def scan(self, name, output):
        i = self.slot.get(name)
        seen, ts = set(), []
        for t in self.tensors(output):         # a forked output hands the same storage out twice: scanned once
            key = (t.data_ptr(), t.dtype, tuple(t.shape), t.stride())
            if key not in seen:
                seen.add(key)
                ts.append(t)
        if self.discover:                      # the constructor's dry run: note who fires when, launch nothing yet
            if ts:
                self._fired[name] = self._tick()
                self.numel.setdefault(name, sum(t.numel() for t in ts))
            return
        if i is None:
            return
        for t in ts:
            t = t.detach()
            if t.dtype not in (torch.float32, ops.BF16):
                t = t.float()
            ops.act_report(t if t.is_contiguous() else t.contiguous(), self.live[i])

    def _tick(self):
        self._clock += 1
        return self._clock

    def end_discovery(self):
        """The dry run is through: the slots in forward order — the order in which the hooks fired.  A module the step enters
        more than once (the projection head: the text tower's rows early, the video tower's behind the video encoder) stands
        where its LAST call is, so that no row can precede a module whose output it consumed; a watched module the step
        never enters has no slot."""
        self.discover = False
        for pat, hit in self._asked.items():   # a request that can never report anything is refused, not dropped
            if not any(n in self._fired for n in hit):
                self.remove()
                raise ValueError(f'activation_report: the step never calls a module matching {pat!r} ({", ".join(hit[:3])}'
                                 f'{", ..." if len(hit) > 3 else ""}): its parent runs it inside a fused kernel, or the '
                                 'recognizer does not use it; watch the parent instead')
        self.names = sorted(self._fired, key=self._fired.get)
        self.slot = {name: i for i, name in enumerate(self.names)}

    def begin_step(self):
        """Ahead of an optimizer step's first forward: the records of the last step make room.  An eager fill on the current
        stream (the forward graph is replayed behind it), once per optimizer step however many forwards that step has."""
        self._depth.clear()
        if self.stale:
            self.live.zero_()
            self.stale = False

    def rows(self, rec, offending_only):
        return [(name, self.numel[name], int(c), int(nf), float(mx))
                for name, nf, mx, c in zip(self.names, rec['nonfinite'].tolist(), rec['max_abs'].tolist(), rec['calls'].tolist())
                if nf or not offending_only]


class CloverEngine:
    def __init__(self, model, sample_batch, lr=5e-5, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.005,
                 paramwise_cfg=None, grad_clip=15.0, max_iters=100000, warmup_iters=0, min_lr_ratio=1e-3,
                 warmup_ratio=1e-3, bucket_mb=64, loss_scale=None, virtual_ranks=1, overflow_report=False,
                 activation_report=False):
        self.model = model
        self.virtual_ranks = int(virtual_ranks)
        # activation_report=True (or dict(modules=[fnmatch patterns over named_modules() names], added to the default
        # block-level list): every forward pass the engine drives folds each watched module's output into a device record —
        # non-finite count, largest finite magnitude — with one clv_act_report launch per output tensor, captured in the
        # forward graphs.  activation_stats() reads the table (the headroom below the 16-bit limit); with overflow_report=True
        # as well a skipped step latches it and overflow_report() names the FIRST module whose output was non-finite.  Off
        # (the default): no hook, no launch, no buffer.
        if activation_report is not False and activation_report is not True and not isinstance(activation_report, dict):
            raise ValueError(f'activation_report must be True, False or dict(modules=[...]), got {activation_report!r}')
        if isinstance(activation_report, dict) and set(activation_report) - {'modules'}:
            raise ValueError(f'activation_report: unknown keys {sorted(set(activation_report) - {"modules"})} (known: modules)')
        self._act = None                       # the _ActivationWatch, built below once the device is known
        # overflow_report=True: every optimizer step also launches clv_grad_report in its "on skip" mode over the gradients —
        # two kernels per slab that return at once unless the step was skipped; overflow_report() then names the
        # parameters that held the non-finite values.  Off (the default): the step launches what it always launched.
        self._overflow_report = bool(overflow_report)
        self._report_tables = None             # per segment ops.GradReportTable, built on first use
        self._report_out = None                # per segment: the report of the last skipped step (overflow_report=True)
        self._stats_out = None                 # per segment: what grad_stats() writes
        # Loss scaling (mmcv_Fp16OptimizerHook.py:33-50,96-149; `fp16 = dict(loss_scale='dynamic')` in the headline config,
        # pretrain_webvid_cc3m.py:21).  `loss_scale` takes what the hook takes: a float (static), 'dynamic'
        # (LossScaler(mode='dynamic'): 2**32, factor 2, window 1000) or a dict of LossScaler arguments; None = the build's
        # default (_lib.LOSS_SCALE / CLOVER_LOSS_SCALE: static 1024 for fp16, none for bf16).  The scaler lives on the DEVICE
        # next to the optimizer's scalars (ops.optim_state_set_scaler): the recognizer multiplies the root gradient of every
        # backward by it (BaseRecognizer._parse_losses reads model._clv_loss_scale_dev), the gradients in the slabs are
        # scaled, clv_optim_prep divides the scale out of the norm and the update, skips the step on an overflow and moves a
        # dynamic scale — no host round trip, and a captured step follows the scale without re-capture.
        from . import _lib as _clv_lib
        if loss_scale is None:
            loss_scale = _clv_lib.LOSS_SCALE_SPEC
        if loss_scale == 'dynamic':
            self.scaler_cfg = dict(init_scale=2.0 ** 32, mode='dynamic', scale_factor=2.0, scale_window=1000)
        elif isinstance(loss_scale, dict):
            self.scaler_cfg = dict(dict(init_scale=2.0 ** 32, mode='dynamic', scale_factor=2.0, scale_window=1000), **loss_scale)
        elif isinstance(loss_scale, (int, float)):
            self.scaler_cfg = dict(init_scale=float(loss_scale), mode='static', scale_factor=2.0, scale_window=1000)
        else:
            raise ValueError(f'loss_scale must be of type float, dict, or "dynamic", got {loss_scale}')
        assert self.scaler_cfg['mode'] in ('dynamic', 'static'), 'mode can only be dynamic or static'
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.base_lr, self.betas, self.eps = lr, betas, eps
        self.grad_clip = grad_clip
        self.max_iters, self.warmup_iters = max_iters, warmup_iters
        self.min_lr_ratio, self.warmup_ratio = min_lr_ratio, warmup_ratio
        self.step_count = 0                    # optimizer_step() calls (taken or skipped)
        self._stale_cleared = False            # finish_backward() cleared the unreached first-touch slots of this step
        self.lr_iter = 0                       # index into the LR schedule when no runner drives it (set_lr)
        self._lr_external = None
        self.last_lr = None                    # what the last optimizer_step() used
        self.graph = None                      # None: the step runs eagerly; else the forward graph step() replays
        self._captures = {}                    # batch-shape signature -> its _Capture
        self._active, self._active_sig = None, None        # the selected _Capture (also while ``graph`` is None)
        self._bwd_text_stream = None           # data-parallel: the stream the text encoder's backward graph replays on
        self._ema_table = None                 # ops.EmaTable once ema_enable() ran
        self._ema_skip_buffers = False
        self.ema_names = {}                    # state_dict name -> its ``ema_*`` buffer name
        self.ema_swapped = False               # True: the parameters hold the average, the ``ema_*`` buffers the weights
        self._vr_emb, self._vr_emb_recomputed = None, {}   # virtual ranks: the last step's stashed embeddings
        self._vr_keep_recomputed = False       # tests: keep the embeddings the recomputed forwards produce
        self._one = None                       # cached root gradient of an unscaled loss
        # Phase clock of the graphed step (bench.py --phases): events on the main stream at the phase boundaries — the
        # forward graph, the eager loss section, the backward graphs, reducer.finish() + optimizer.  GPU time between
        # consecutive marks, averaged by phase_ms(); off (None) unless start_phase_timing() was called.
        self._phase_ev = None
        # the recognizer names the batch entries its rank-local part consumes (CloverPretrain: captions + both
        # masks; CloverFinetune retrieval: captions only)
        self._encode_keys = tuple(getattr(model, 'CLV_ENCODE_KEYS', ('token_ids', 'input_mask', 'mlm_label', 'v_token_mask')))
        self._loss_takes_gathered = (hasattr(model, 'contrastive_losses')
                                     and 'gathered' in inspect.signature(model.contrastive_losses).parameters)
        self._encode_takes_text_cut = hasattr(model, 'encode') and 'text_cut' in inspect.signature(model.encode).parameters
        device = next(model.parameters()).device
        if device.type != 'cuda':
            raise RuntimeError('CloverEngine drives the HIP kernels: move the model to an MI355X first (there is no '
                               f'CPU path; got parameters on {device})')
        self._device = device
        if self.virtual_ranks < 1:
            raise ValueError(f'virtual_ranks must be >= 1, got {virtual_ranks}')
        if self.virtual_ranks > 1:
            self._check_virtual_ranks(model, sample_batch)
        pw = paramwise_cfg or dict(norm_decay_mult=0.0, bias_decay_mult=0.0,
                                   custom_keys={'absolute_pos_embed': dict(decay_mult=0.),
                                                'relative_position_bias_table': dict(decay_mult=0.)})
        opt_map = paramwise_options(model, weight_decay, pw)       # name -> (weight_decay, lr_mult)

        # ---- dry run: which parameters does the step graph actually reach?
        model.zero_grad(set_to_none=True)
        if activation_report is not False:
            # hooked BEFORE the dry run: the order in which the hooks fire there is the table's forward order
            # (_ActivationWatch.end_discovery), and every forward graph captured later holds the scans
            self._act = _ActivationWatch(model, activation_report, device)
        with self._act_forward():
            out = model.train_step(sample_batch, None)
        if self._act is not None:
            self._act.end_discovery()
        out['loss'].backward()
        used = [(n, p) for n, p in model.named_parameters() if p.requires_grad and p.grad is not None]
        name_of = {id(p): n for n, p in model.named_parameters()}
        self.unused_names = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
        model.zero_grad(set_to_none=True)

        # reverse registration order ~ order in which backward produces the gradients
        used = list(reversed(used))
        # modules that apply several parameters as one GEMM ask for adjacent slab slots (clv_fuse_groups())
        groups = []
        used_ids = {id(p) for _, p in used}
        for mod in model.modules():
            for grp in (mod.clv_fuse_groups() if hasattr(mod, 'clv_fuse_groups') else []):
                if all(id(q) in used_ids for q in grp) and len({opt_map[name_of[id(q)]] for q in grp}) == 1:
                    groups.append((mod, grp))
        member = {id(q): gi for gi, (_, grp) in enumerate(groups) for q in grp}
        ordered, placed = [], set()
        for n, p_ in used:
            gi = member.get(id(p_))
            if gi is None:
                ordered.append((n, p_))
            elif gi not in placed:
                placed.add(gi)
                ordered.extend((name_of[id(q)], q) for q in groups[gi][1])
        used = ordered
        # one slab per distinct (weight_decay, lr_mult): the reference config has two (decayed weights; norm / bias /
        # position-table parameters without decay), any other decay_mult / lr_mult of a paramwise_cfg adds its own
        classes = {}
        for n, p_ in used:
            classes.setdefault(opt_map[n], []).append((n, p_))
        self.segments = [_Segment(members, wd, device, lr_mult=lm)
                         for (wd, lm), members in sorted(classes.items(), key=lambda kv: (-kv[0][0], kv[0][1]))]
        # gradient-norm accumulator: [0] the sum of squares the norm kernels add to; from float 16 on, the CLV_SUMSQ_SLOTS
        # partial sums (64 bytes apart) that the weight-gradient kernels fill in fused-norm mode (_setup_fused_norm)
        self.sumsq = torch.zeros(16 + 16 * ops.SUMSQ_SLOTS, device=device, dtype=torch.float32)
        self._norm_tables = None               # per segment (table, blocks) of what the norm pass still reads; None: whole slabs
        self.optim_state = ops.optim_state_new(device)
        self._scaler_on = self.scaler_cfg['mode'] == 'dynamic' or self.scaler_cfg['init_scale'] != 1.0
        if self._scaler_on:
            ops.optim_state_set_scaler(self.optim_state, self.scaler_cfg['init_scale'], self.scaler_cfg['mode'] == 'dynamic',
                                       self.scaler_cfg['scale_factor'], self.scaler_cfg['scale_window'])
        object.__setattr__(model, '_clv_loss_scale_dev', self.optim_state.view(torch.float32)[8] if self._scaler_on else False)     # False: an engine without a scaler
        self.num_params = sum(p.numel() for _, p in used)

        # ---- gradient buckets (contiguous slices of the flat grad buffers) + readiness hooks
        # gradient classes in the order their backward completes: 'h' heads + fusion encoder, 't' text encoder,
        # 'v1' late video stages, 'v0' early video stages + patch embedding (graph mode sends buckets per class)
        self._pclass = {}
        if hasattr(model, 'backbone'):
            for q in model.backbone.parameters():
                self._pclass[id(q)] = 'v0'
            if hasattr(model.backbone, 'late_parameters'):
                for q in model.backbone.late_parameters():
                    self._pclass[id(q)] = 'v1'
        if hasattr(model, 'text_backbone'):
            for q in model.text_backbone.parameters():
                self._pclass[id(q)] = 't'
        # data-parallel jobs exchange the gradients as bf16 (CLOVER_BF16_ALLREDUCE=0: fp32): each bucket's slice is packed
        # into a bf16 wire slab right before its all-reduce and sumsq / AdamW read the reduced bf16 copy — 427 MB instead
        # of 757 MB per step over xGMI at config 2; accumulation in the backward and the update itself stay fp32
        self.wire = None
        if collectives_active() and os.environ.get('CLOVER_BF16_ALLREDUCE', '1') == '1':
            self.wire = [torch.zeros_like(seg.flat_g, dtype=ops.BF16) for seg in self.segments]
        self.reducer = BucketedGradReducer([(seg.flat_g, seg.params, seg.offsets) for seg in self.segments],
                                           bucket_bytes=bucket_mb << 20,
                                           split_key=lambda q: self._pclass.get(id(q), 'h'), wire=self.wire)
        per_mod = {}
        for mod, grp in groups:
            seg = next(sg for sg in self.segments if any(q is grp[0] for q in sg.params))
            per_mod.setdefault(id(mod), (mod, []))[1].append(seg.fused_view(grp))
        for mod, views in per_mod.values():
            mod._clv_fused = views                       # same order as clv_fuse_groups()
        for seg in self.segments:
            seg.build_transposed()
        self._zero_views = None                # None: clear whole slabs
        self._fresh_sinks = {}                 # id(sink) -> (sink, segment index, slab offset, numel) of the first-touch slots
        self._ft, self.first_touch_params = ops.FirstTouch(), 0
        self._norm_state = ops.FusedNormState()
        self._setup_first_touch(sample_batch)
        self._setup_fused_norm()
        if self._overflow_report:
            self._report_out = [ops.grad_report_new(tab, device) for tab in self._grad_report_tables()]

    def _check_virtual_ranks(self, model, sample_batch):
        """What a virtual-rank step cannot reproduce is refused with its reason."""
        k = self.virtual_ranks
        if not isinstance(sample_batch, dict):
            raise ValueError(f'virtual_ranks={k}: sample_batch is ONE micro-batch (a dict), the geometry of all {k}')
        if collectives_active():
            raise NotImplementedError(f'virtual_ranks={k} in a data-parallel job: virtual ranks times real ranks is not '
                                      'implemented (the global batch would be world * k * B rows)')
        if getattr(model, 'is_qa', False):
            raise NotImplementedError(f'virtual_ranks={k}: the video_qa / FIB tasks have no loss shared between samples, '
                                      'so there is nothing a larger global batch would change')
        if not hasattr(model, 'encode') or not hasattr(model, 'contrastive_losses'):
            raise NotImplementedError(f'virtual_ranks={k} needs a recognizer with the encode / contrastive_losses split '
                                      f'(CloverPretrain, CloverFinetune(task="retrieval")); got {type(model).__name__}')
        from .nn import BatchNorm1d
        bn = [n for n, m in model.named_modules() if isinstance(m, BatchNorm1d)]
        if bn:
            raise NotImplementedError(f'virtual_ranks={k}: {bn[0]} is a BatchNorm1d; per-micro-batch statistics are not the '
                                      "reference's SyncBN over the global batch, and the recomputed forward would move the "
                                      'running statistics twice')

    def _setup_fused_norm(self):
        """One-rank jobs: the first-touch weight gradients (most of the parameters: each is written by exactly one launch per
        step) deliver their sum of squares from the kernel that writes them (ops.linear_wgrad: flag bit 2 of the grouped /
        fold launches, an explicit pass on any other path), so the norm pass before the clip reads only the REST of the
        slabs — `clv_sumsq_ranges` over the complement — instead of all 0.76 GB.  Not in data-parallel jobs: their norm is
        that of the REDUCED gradients (mmcv_Fp16OptimizerHook.py:119-131).  CLOVER_FUSED_NORM=0 switches it off."""
        fresh = self._fresh_sinks
        if (not fresh or self.reducer.active or self.wire is not None or os.environ.get('CLOVER_FUSED_NORM', '1') != '1'
                or not self.segments[0].flat_g.is_cuda or self.virtual_ranks > 1):
            return
        slots = self.sumsq[16:]
        tables = []
        for si, seg in enumerate(self.segments):
            spans = sorted((off, off + n) for _, sj, off, n in fresh.values() if sj == si)
            tables.append(ops.sumsq_range_table(_complement(spans, seg.flat_g.numel()), seg.flat_g.device))
        for sk, _, _, _ in fresh.values():
            sk._clv_ssq = ops.NormSlots(self.sumsq, slots, self._norm_state)
        self._norm_tables = tables

    # ------------------------------------------------------------------ gradient clearing
    def _setup_first_touch(self, sample_batch):
        """Decide which weight gradients are never cleared.  A Linear weight whose gradient reaches its slab slot through
        exactly ONE weight-gradient launch per step (ops.linear_wgrad) needs neither the zero-fill after the optimizer
        nor the read of a "+=": that launch STORES (ops.first_touch) — 8 B of HBM traffic per parameter and step less on
        most of the 189 M parameters.  Which slots qualify is MEASURED, not declared: a reference backward into cleared
        slabs, then the same backward (same RNG state) into slabs poisoned with NaN with every once-written sink marked
        first-touch; a slot qualifies when it comes out finite and equal to the reference (a gradient that also arrives
        through autograd BEFORE its launch, or a sink the launch does not recognise, fails here and keeps being cleared).
        A third pass with the final marking must reproduce every gradient, otherwise the scheme is switched off."""
        if os.environ.get('CLOVER_GRAD_FIRST_TOUCH', '1') != '1' or self.virtual_ranks > 1:
            return                             # (virtual ranks: k backward passes ADD into the slabs, nothing may store)
        sinks = {}                             # data_ptr -> (sink tensor, segment index, slab offset, numel)
        for si, seg in enumerate(self.segments):
            for q, off in zip(seg.params, seg.offsets):
                sk = getattr(q, '_clv_pad_grad', None)         # a phantom-padded parameter's kernels write the padded view
                sk = sk if sk is not None else q._clv_grad
                sinks[sk.data_ptr()] = (sk, si, off, sk.numel())
            for f in seg._fused:               # a fused view starts where its first member does: the view is what ops sees
                sinks[f._clv_grad.data_ptr()] = (f._clv_grad, si, f._clv_off, f.numel())
        cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
        drop_ctr = ops._dropout_counter(self.segments[0].flat_g.device)      # the kernels' own dropout seeds
        drop_ctr0 = drop_ctr.clone()

        def mark(ptrs):
            for t, _, _, _ in sinks.values():
                t._clv_ft = None
            for ptr in ptrs:
                sinks[ptr][0]._clv_ft = self._ft
            self._ft.on = bool(ptrs)
            self._ft.done.clear()

        def span(slabs, ptr):
            _, si, off, n = sinks[ptr]
            return slabs[si][off:off + n]

        def run(ptrs):
            torch.set_rng_state(cpu_rng)
            torch.cuda.set_rng_state(gpu_rng)
            drop_ctr.copy_(drop_ctr0)
            for seg in self.segments:
                seg.flat_g.zero_()
            mark(ptrs)
            for ptr in ptrs:
                span([seg.flat_g for seg in self.segments], ptr).fill_(float('nan'))
            out = self.model.train_step(sample_batch, None)
            self._backward(lambda: out['loss'].backward())
            return [seg.flat_g.clone() for seg in self.segments]

        def same(a, b):
            return bool(torch.isfinite(a).all()) and float((a - b).norm()) <= 1e-4 * float(b.norm()) + 1e-12

        hooks_were = self.reducer.enabled
        self.reducer.enabled = False
        ok = []
        try:
            ops.FRESH_LOG = {}
            ref = run([])
            log, ops.FRESH_LOG = ops.FRESH_LOG, None
            cand = [ptr for ptr, (calls, numel) in log.items() if calls == 1 and ptr in sinks and sinks[ptr][3] == numel]
            # exactly three passes on every rank, whatever they find: the step contains collectives (feature all-gather)
            got = run(cand)
            ok = [ptr for ptr in cand if same(span(got, ptr), span(ref, ptr))]
            got = run(ok)
            if not all(same(g, r) for g, r in zip(got, ref)):
                ok = []
        finally:
            ops.FRESH_LOG = None
            self.reducer.reset()
            self.reducer.enabled = hooks_were
            torch.set_rng_state(cpu_rng)
            torch.cuda.set_rng_state(gpu_rng)
            drop_ctr.copy_(drop_ctr0)
        mark(ok)
        self._clear_all()
        if not ok:
            return
        # what is still cleared every step: the complement of the first-touch slots, as few contiguous views as possible
        self._fresh_sinks = {id(sinks[ptr][0]): sinks[ptr] for ptr in ok}
        self._zero_views = []
        for si, seg in enumerate(self.segments):
            spans = sorted((off, off + n) for _, sj, off, n in self._fresh_sinks.values() if sj == si)
            self._zero_views += [seg.flat_g[a:b] for a, b in _complement(spans, seg.flat_g.numel())]
        self.first_touch_params = sum(n for _, _, _, n in self._fresh_sinks.values())

    def _clear_all(self):
        """All gradients and norm partial sums clear, every first-touch slot stale: what a fresh step starts from.  For
        set-up, dry_step() and capture(); between steps zero_grads() clears only what needs it."""
        for seg in self.segments:
            seg.flat_g.zero_()
        self.sumsq.zero_()
        self._norm_state.dirty = False
        self._ft.done.clear()

    def zero_grads(self):
        """Clear the gradients for the next backward: zero-fill what accumulates, mark the first-touch slots stale."""
        self._ft.done.clear()
        if self._zero_views is None:
            for seg in self.segments:
                seg.flat_g.zero_()
            return
        views = self._zero_views + (self._active.stale_views if self._active is not None else [])
        if self._norm_tables is not None:
            views = views + [self.sumsq]       # a backward without an optimizer step (dry run, warm-up) left partial sums
        if views:
            torch._foreach_zero_(views)

    def _stale_sinks(self):
        """First-touch slots the last backward did NOT write (a weight the batch did not reach): their content is the
        previous step's gradient — they must be cleared like the others."""
        if self._zero_views is None:
            return []
        return [self.segments[si].flat_g[off:off + n]
                for key, (_, si, off, n) in self._fresh_sinks.items() if key not in self._ft.done]

    # ------------------------------------------------------------------ one step
    def current_lr(self):
        """LR of the NEXT optimizer step.  Under a runner the schedule is indexed by the runner's ``iter`` — batch
        indices, which the two-loader mode advances once per TWO optimizer steps (clover_runner.py:76-91) — and set
        through ``set_lr`` by ``runner.LrUpdaterHook`` as mmcv's LR hook does in ``before_train_iter``.  Stand-alone
        (bench.py) the engine indexes the same schedule by its own count of steps, starting at 0 like mmcv's iter."""
        if self._lr_external is not None:
            return self._lr_external
        return cosine_lr(self.base_lr, self.lr_iter, self.max_iters, self.min_lr_ratio, self.warmup_iters,
                         self.warmup_ratio)

    def set_lr(self, lr):
        """Externally scheduled learning rate, used by every following step until changed (None: own schedule)."""
        self._lr_external = None if lr is None else float(lr)

    def dry_step(self, batch):
        """forward + backward + gradient exchange WITHOUT the optimizer: warms the kernels, the GEMM tuner and the
        gradient reducer's hook calibration and leaves weights, Adam moments, step counts and the LR index untouched
        (gradients are zeroed again)."""
        self._ft.done.clear()
        self._act_begin_step()
        with self._act_forward():
            out = self.model.train_step(batch, None)
        self._backward(lambda: out['loss'].backward())
        self.finish_backward()
        self._stale_cleared = False
        self._clear_all()
        self._act_end_step()
        return out

    def step(self, batch):
        """forward + backward + gradient all-reduce + clip + AdamW.  Returns train_step's dict.  With ``virtual_ranks=k``
        ``batch`` is a sequence of k micro-batches of one geometry (forward_backward)."""
        self._refuse_swapped('step')
        out = self.forward_backward(batch)
        self.optimizer_step()
        self._mark('optimizer')
        return out

    def _select(self, batch):
        """Make the captured step of ``batch``'s geometry the active one.  The reference alternates 8-frame video and
        1-frame image batches (clover_runner.py:76-93): one set of graphs per geometry, captured on first sight."""
        sig = self._signature(batch)
        if sig != self._active_sig:
            if sig in self._captures:
                self._activate(sig)
            else:
                self.capture(batch)

    def _forward_backward_one(self, batch):
        """Forward and backward of a single batch, graphed or eager, up to and including finish_backward()."""
        self.reducer.begin_step()
        if self.graph is not None:
            self._select(batch)
            self._act_begin_step()             # behind a first-sight capture, whose warm-up passes fold into the table too
            out = self._graphed_forward_backward(batch)
        else:
            self.reducer.prepacked = frozenset()
            self._ft.done.clear()
            self._act_begin_step()
            with self._act_forward():
                out = self.model.train_step(batch, None)
            self._backward(lambda: out['loss'].backward())
        self.finish_backward()
        return out

    # ------------------------------------------------------------------ virtual ranks
    def forward_backward(self, batches):
        """Everything of step() except optimizer_step(); returns train_step's dict.

        ``virtual_ranks=k``: ``batches`` is a sequence of k batch dicts of one geometry; micro-batch j is rows
        [j B, (j + 1) B) of the global batch, rank-major as all_gather orders them.  The step computes what a k-rank DDP job
        of the reference computes: the contrastive / rank losses ONCE on all k B rows, each micro-batch's rank-local loss
        (mlm_loss) on its own rows, and the gradient  1/k sum_j [J_j^T dLc/dE[jB:(j+1)B] + grad L_local,j]  — including the
        1/W effect of the gather's local-slice backward.  A micro-batch is a rank whose all-gather is a copy:

        * pass 1: every micro-batch runs ``encode`` (the captured forward graph, or eagerly under no_grad); its embeddings
          and local loss are stashed, and so is the RNG state its dropout / DropPath draws start from;
        * the loss section runs once, eagerly, on the [k B, 6, D] stash, with the device loss scale as root gradient;
        * pass 2: the last micro-batch's activations are still alive, so it goes backward at once; every other one restores
          its RNG state, recomputes its forward (same masks) and goes backward with its slice of d E.  All k backward passes
          ADD into the gradient slabs (an engine with virtual ranks has neither first-touch stores nor the fused norm), and
          ``optimizer_step`` divides by k next to the loss scale.

        Afterwards the slab views (``param.grad``) hold loss_scale * sum_j.  Logged values are what rank 0 of the reference
        logs after its all-reduce: the shared contrastive values, the mean of the k local ones, ``loss`` their sum;
        ``num_samples`` counts the k B samples of the step."""
        self._refuse_swapped('forward_backward')
        if self.virtual_ranks == 1:
            return self._forward_backward_one(batches if isinstance(batches, dict) else batches[0])
        k = self.virtual_ranks
        if isinstance(batches, dict) or len(batches) != k:
            raise ValueError(f'virtual_ranks={k}: a step takes a sequence of {k} micro-batches, got '
                             + ('one batch dict' if isinstance(batches, dict) else f'{len(batches)}'))
        sig = self._signature(batches[0])
        for j in range(1, k):
            if self._signature(batches[j]) != sig:
                raise ValueError(f'virtual_ranks={k}: micro-batch {j} has another geometry than micro-batch 0 '
                                 f'({self._signature(batches[j])} vs {sig}); the k micro-batches share one set of graphs')
        self.reducer.begin_step()
        self.reducer.prepacked = frozenset()
        graphed = self.graph is not None
        if graphed:
            self._select(batches[0])
        self._act_begin_step()                 # all 2k - 1 forwards of the step fold into the same records
        model, cap = self.model, self._active
        drop_ctr = ops._dropout_counter(self._device)

        def rng_save():
            return torch.cuda.get_rng_state(self._device), drop_ctr.clone()

        def rng_restore(st):
            torch.cuda.set_rng_state(st[0], self._device)
            drop_ctr.copy_(st[1])

        def forward(j, grad):
            """encode of micro-batch j -> (emb, mlm): the static outputs of the forward graph, or eager tensors."""
            b = batches[j]
            if graphed:
                for name, v in cap.batch.items():
                    if b[name] is not v:
                        v.copy_(b[name], non_blocking=True)
                self.graph.replay()
                return cap.emb, cap.mlm
            with torch.enable_grad() if grad else torch.no_grad(), self._act_forward():
                return model.encode(b['imgs'], **{name: b[name] for name in self._encode_keys})

        def backward(live, demb, dmlm):
            if graphed:
                cap.demb.copy_(demb)
                if cap.dmlm is not None:
                    cap.dmlm.copy_(dmlm)
                self._replay_backward()
            else:
                emb, mlm = live
                roots, grads = [emb], [demb.to(emb.dtype)]
                if mlm is not None:
                    roots.append(mlm)
                    grads.append(dmlm.to(mlm.dtype).reshape(mlm.shape))
                self._backward(lambda: torch.autograd.backward(roots, grads))

        # ---- pass 1
        rng, embs, mlms, live = [], [], [], None
        for j in range(k):
            rng.append(rng_save())
            live = forward(j, grad=j == k - 1)
            embs.append(live[0].detach().float().clone() if graphed else live[0].detach().float())
            if live[1] is not None:
                mlms.append(live[1].detach().float().reshape(()).clone())
        rng_end = rng_save()
        self._vr_emb = embs
        # ---- the loss section, once, on all k * B rows
        E = torch.cat(embs, 0).requires_grad_()
        mlm = torch.stack(mlms).mean().requires_grad_() if mlms else None     # rank 0 logs the mean of the k local values
        if self._loss_takes_gathered:
            losses = model.contrastive_losses(None, mlm, gathered=E)
        else:
            losses = model.contrastive_losses(E, mlm)
        loss, log_vars = self._parse_root_scaled(losses)
        loss.backward(gradient=self._root_gradient(loss))
        B = embs[0].shape[0]
        dE = E.grad
        dmlm = mlm.grad if mlm is not None else None          # d loss / d L_local,j = the root gradient, for every j
        # ---- pass 2: the live micro-batch first, then every other one recomputed under its own masks
        self._vr_emb_recomputed = {}
        for j in [k - 1] + list(range(k - 1)):
            if j != k - 1:
                rng_restore(rng[j])
                live = forward(j, grad=True)
                if self._vr_keep_recomputed:
                    self._vr_emb_recomputed[j] = live[0].detach().float().clone()
            backward(live, dE[j * B:(j + 1) * B], dmlm)
            live = None
        rng_restore(rng_end)                                   # the next step draws new masks, not micro-batch 1's again
        self.finish_backward()
        return dict(loss=loss.detach(), log_vars=log_vars, num_samples=k * len(next(iter(batches[0].values()))))

    def finish_backward(self):
        """Close a backward pass: clear the first-touch slots an EAGER backward did not reach, THEN complete the gradient
        exchange.  The order matters in data-parallel mode: ``reducer.finish()`` packs and all-reduces the
        bucket of an unreached parameter, and the norm / AdamW kernels read the reduced wire copy — a slot cleared after
        the exchange would still update the weight with the previous step's gradient.  (A captured geometry's unreached
        slots are cleared with the rest of the gradients after every optimizer step: ``stale_views``.)  A caller that
        drives its own ``loss.backward()`` calls this instead of ``reducer.finish()``."""
        if self.graph is None:
            stale = self._stale_sinks()
            if stale:
                torch._foreach_zero_(stale)
            self._stale_cleared = True
        self.reducer.finish()

    def _backward(self, run):
        """Run a backward pass / segment with the weight-gradient folds deferred to ONE batched launch at its end —
        unless gradient-ready hooks put buckets on the wire from inside the pass (eager data-parallel mode), where a
        gradient must be final when its hook fires."""
        if self.reducer.active and self.reducer.enabled:
            run()
        else:
            with ops.defer_folds():
                run()

    # ------------------------------------------------------------------ hipGraph mode
    def _parse_root_scaled(self, losses, **kw):
        """model._parse_losses for a backward the engine starts itself: the loss scale is handed to autograd as the ROOT
        gradient (_root_gradient) instead of through the recognizer's scaling node — one dependent launch less on the
        step's serial chain (same-box 10.29-10.31 -> see DESIGN §5)."""
        object.__setattr__(self.model, '_clv_root_scaled', True)
        try:
            return self.model._parse_losses(losses, **kw)
        finally:
            object.__setattr__(self.model, '_clv_root_scaled', False)

    def _root_gradient(self, loss):
        """d loss / d loss of an engine-started backward: the device-resident loss scale (a 0-dim view of the optimizer
        record: read when the kernels run, so a captured section follows a moving scale), or a cached 1."""
        if self._scaler_on:
            return self.model._clv_loss_scale_dev
        if self._one is None or self._one.device != loss.device or self._one.dtype != loss.dtype:
            self._one = torch.ones_like(loss)
        return self._one

    @staticmethod
    def _signature(batch):
        return tuple((k, tuple(v.shape)) for k, v in sorted(batch.items()))

    def _activate(self, sig):
        cap = self._active = self._captures[sig]
        self._active_sig, self.graph = sig, cap.graph
        # The previous optimizer step cleared the stale views of the geometry that ran THEN.  A first-touch slot that
        # geometry writes and this one never does still holds that step's gradient: clear this geometry's stale slots
        # before its first replay (afterwards zero_grads() keeps them clear while it stays active).
        if cap.stale_views:
            torch._foreach_zero_(cap.stale_views)

    def input_buffers(self, shapes=None):
        """The static input tensors of the active hipGraphs (None before capture): a loader that writes its host-to-device
        copies straight into them — and hands the same dict to step() — saves the per-step staging copy.  With ``shapes``
        ({key: shape} of a batch): those of the capture of THAT geometry, active or not, or None when it has none yet
        (a loader of one of two alternating streams asks for its own, utils/packed_loader.py)."""
        if self.graph is None:
            return None
        if shapes is None:
            return self._active.batch
        cap = self._captures.get(tuple((k, tuple(s)) for k, s in sorted(shapes.items())))
        return cap.batch if cap is not None else None

    def _graphed_forward_backward(self, batch):
        """encode (hipGraph) -> gather + contrastive losses (eager: it holds the step's only forward
        collective) -> backward of the losses (eager, a handful of kernels) -> encode backward (hipGraph)."""
        cap = self._active
        for k, v in cap.batch.items():
            if batch[k] is not v:
                v.copy_(batch[k], non_blocking=True)
        self._mark('start')
        self.graph.replay()
        self._mark('forward')
        if cap.graph_loss is not None:
            # the loss section as a graph of its own: only the feature all-gather (and the all-reduce of the logged
            # scalars) stay eager — ~60 launch-bound kernels otherwise paced by the host
            g_static, names, packed, loss = cap.loss_io
            with torch.no_grad():
                if collectives_active():
                    from .utils.gather_loss import gather_rows
                    g_static.copy_(gather_rows(cap.emb.float(), equal_sizes=True))
                else:
                    g_static.copy_(cap.emb)
            cap.graph_loss.replay()
            if collectives_active():
                packed = packed / self.world
                dist.all_reduce(packed)
            else:
                packed = packed.clone()        # the graph's static output: the next replay overwrites it
            from .recognizers.base import LazyLogVars
            log_vars = LazyLogVars(names, packed)
            loss = loss.detach().clone()
        else:
            emb = cap.emb.detach().requires_grad_()
            mlm = cap.mlm.detach().requires_grad_() if cap.mlm is not None else None
            losses = self.model.contrastive_losses(emb, mlm)
            loss, log_vars = self._parse_root_scaled(losses)
            loss.backward(gradient=self._root_gradient(loss))
            cap.demb.copy_(emb.grad)
            if mlm is not None:
                cap.dmlm.copy_(mlm.grad)
        self._mark('loss')
        self._replay_backward()
        self._mark('backward')
        return dict(loss=loss.detach(), log_vars=log_vars, num_samples=len(next(iter(batch.values()))))

    def start_phase_timing(self):
        self._phase_ev = []

    def _mark(self, name):
        if self._phase_ev is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self._phase_ev.append((name, e))

    def phase_ms(self):
        """Mean GPU milliseconds per phase since start_phase_timing() (call after a device sync); stops the clock."""
        ev, self._phase_ev = self._phase_ev, None
        tot, cnt = {}, {}
        for (_, a), (n, b) in zip(ev, ev[1:]):
            if n != 'start':
                tot[n] = tot.get(n, 0.0) + a.elapsed_time(b)
                cnt[n] = cnt.get(n, 0) + 1
        return {n: tot[n] / cnt[n] for n in tot}

    def _ready(self, *classes):
        cl = self._pclass
        return lambda q: cl.get(id(q), 'h') in classes

    def _replay_backward(self):
        cap = self._active
        self.reducer.prepacked = cap.prepacked
        cap.graph_bwd.replay()
        if cap.graph_bwd_video is None:
            return
        # Data-parallel mode: the backward is cut at the encoders' outputs (and once inside the video encoder).  The
        # heads / fusion gradients are complete now: put their buckets on the wire.  Then the text encoder's
        # backward (its own graph, on its own stream) and the video encoder's backward run CONCURRENTLY — as they do
        # inside the single backward graph of a 1-GPU job — and each gradient class's buckets leave as soon as its
        # graph is through: the text encoder's under the rest of the video backward, the late video stages'
        # (most of the encoder's parameters, little of its time) under the token-heavy early stages;
        # step() -> reducer.finish() sends what is left (early stages + patch embedding: a few MB).
        main = torch.cuda.current_stream()
        ts = self._bwd_text_stream if cap.graph_bwd_text is not None else None
        self.reducer.launch_where(self._ready('h'))
        if ts is not None:
            ts.wait_stream(main)
            with torch.cuda.stream(ts):
                cap.graph_bwd_text.replay()
                self.reducer.launch_where(self._ready('h', 't'))
        for i, g in enumerate(cap.graph_bwd_video):
            g.replay()
            if i + 1 < len(cap.graph_bwd_video):           # came down to the in-encoder cut
                self.reducer.launch_where(self._ready('h', 'v1') if ts is not None else self._ready('h', 't', 'v1'))
        if ts is not None:
            main.wait_stream(ts)

    def capture(self, batch, warmup=2):
        """Capture the rank-local part of the step — CloverPretrain.encode and its backward, ~2300 of
        the ~2400 kernel launches — as two hipGraphs sharing one memory pool (static shapes; no
        data-dependent shape and no host sync by construction).  The cross-rank part (feature
        all-gather, InfoNCE/rank losses, logged-scalar all-reduce) stays eager between the two
        replays, so no RCCL call is ever captured and the same code path serves 1..8 GPUs."""
        model = self.model
        sb = {k: v.clone() for k, v in batch.items()}
        cut_ok = self.reducer.active and hasattr(model, 'backbone')
        text_ok = cut_ok and hasattr(model, 'text_backbone') and self._encode_takes_text_cut
        if text_ok and self._bwd_text_stream is None:
            self._bwd_text_stream = torch.cuda.Stream()

        def encode(vcuts=None, tcuts=None):      # (the recognizer may return no rank-local loss: mlm is None)
            kw = {k: sb[k] for k in self._encode_keys}
            if text_ok:
                kw['text_cut'] = tcuts
            return model.encode(sb['imgs'], video_cut=vcuts, **kw)

        def roots(emb, mlm, demb, dmlm):
            return [emb] + ([mlm] if mlm is not None else []), [demb] + ([dmlm] if mlm is not None else [])

        def bwd_cut(cuts):
            self._backward(lambda: torch.autograd.backward([o for o, _ in cuts], [leaf.grad for _, leaf in cuts]))

        def bwd_video(cuts):                   # output cut first, then the in-encoder cut (backward order)
            for c in reversed(cuts):
                bwd_cut([c])
        self.reducer.enabled = False           # no collective may be issued from inside a capture; in graph
        self.reducer.reset()                   # mode the engine launches the buckets between / after the replays
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                vcuts = [] if cut_ok else None
                tcuts = [] if text_ok else None
                self._ft.done.clear()
                with self._act_forward():
                    emb, mlm = encode(vcuts, tcuts)
                self._backward(lambda: torch.autograd.backward(*roots(emb, mlm, torch.zeros_like(emb),
                                                                      torch.zeros_like(mlm) if mlm is not None else None)))
                if vcuts:
                    bwd_video(vcuts)
                if tcuts:
                    bwd_cut(tcuts)
        torch.cuda.current_stream().wait_stream(side)
        # no autograd graph may survive into the capture: a live one pins the parameters'
        # AccumulateGrad nodes to the warm-up stream and their accumulation escapes the hipGraph
        del emb, mlm, vcuts, tcuts
        self._clear_all()                     # the captured backward holds the first-touch stores of a fresh step
        torch.cuda.synchronize()
        gf, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        gb2 = None
        gb3 = torch.cuda.CUDAGraph() if text_ok else None
        # thread_local: RCCL's watchdog thread (W > 1) keeps polling events while we capture
        vcuts = [] if cut_ok else None
        tcuts = [] if text_ok else None
        with torch.cuda.graph(gf, capture_error_mode='thread_local'), self._act_forward():
            emb, mlm = encode(vcuts, tcuts)                # (the watched modules' scans are nodes of this graph)
        demb = torch.zeros_like(emb)
        dmlm = torch.zeros_like(mlm) if mlm is not None else None
        # Data-parallel jobs: the bf16 wire copy of every bucket is written INSIDE the backward graph that completes its
        # gradients (the pack kernels are plain launches; only the RCCL calls stay between the replays)
        pack = cut_ok
        prepacked = set()
        with torch.cuda.graph(gb, pool=gf.pool(), capture_error_mode='thread_local'):
            self._backward(lambda: torch.autograd.backward(*roots(emb, mlm, demb, dmlm)))
            if pack:
                prepacked |= self.reducer.pack_where(self._ready('h'))
        if cut_ok:
            gb2 = []
            ncut = len(vcuts)
            for i, c in enumerate(reversed(vcuts)):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=gf.pool(), capture_error_mode='thread_local'):
                    bwd_cut([c])
                    if pack:
                        # as _replay_backward launches them: the late video stages after the first cut graph, what is
                        # left of the video encoder (and, without a text cut, of the text encoder) after the last
                        cls = ('v1',) if i + 1 < ncut else (('v0', 'v1') if text_ok else ('v0', 'v1', 't'))
                        prepacked |= self.reducer.pack_where(self._ready(*cls), skip=prepacked)
                gb2.append(g)
        if text_ok:
            # captured LAST and into a pool of its own: it replays concurrently with the video graph, so neither
            # may recycle memory the other still reads (blocks this capture frees return to gf's pool after the
            # video graph has been laid out; its own temporaries never alias the video graph's)
            with torch.cuda.graph(gb3, capture_error_mode='thread_local'):
                bwd_cut(tcuts)
                if pack:
                    prepacked |= self.reducer.pack_where(self._ready('t'), skip=prepacked)
        cap = _Capture(gf, gb, gb2, gb3, batch=sb, emb=emb, mlm=mlm, demb=demb, dmlm=dmlm, cuts=(vcuts, tcuts),
                       stale_views=self._stale_sinks(), prepacked=frozenset(prepacked))
        twice = self._norm_state.dirty
        self._clear_all()                          # a capture pass does not execute kernels; be explicit
        if twice:
            raise RuntimeError('fused gradient norm: the captured backward gives a first-touch sink two gradients; build the '
                               'engine with CLOVER_FUSED_NORM=0')
        cap.graph_loss, cap.loss_io = self._capture_loss_graph(cap)
        self._act_end_step()                       # the warm-up passes folded into the table: the next step starts clean
        # published whole and last: a capture that raised has left the engine's geometries as they were
        sig = self._signature(batch)
        self._captures[sig] = cap
        self._activate(sig)
        return True

    def _capture_loss_graph(self, cap):
        """The section between the two encode graphs — contrastive / rank losses on the gathered embeddings, the loss
        sum and its backward down to d emb / d mlm — as a hipGraph over a static gathered tensor.  The all-gather that
        fills it and the all-reduce of the logged scalars stay eager (no RCCL call is ever captured); the gather's
        backward is the local slice (gather_loss.py:64-72), taken inside the graph.  CLOVER_LOSS_GRAPH=1 is ignored with
        virtual_ranks > 1: that loss section runs once per k replays, on a tensor k times the captured one."""
        model = self.model
        if (os.environ.get('CLOVER_LOSS_GRAPH', '0') != '1' or self.virtual_ranks > 1 or not self._loss_takes_gathered
                or not getattr(getattr(model, 'ssl_loss', None), 'equal_batch', False)):
            return None, None
        emb = cap.emb
        B = emb.shape[0]
        g_static = torch.zeros((self.world * B,) + tuple(emb.shape[1:]), device=emb.device, dtype=torch.float32)
        g_static[self.rank * B:(self.rank + 1) * B].copy_(emb)
        out = {}

        def run():
            g = g_static.detach().requires_grad_()
            mlm = cap.mlm.detach().requires_grad_() if cap.mlm is not None else None
            losses = model.contrastive_losses(None, mlm, gathered=g)
            loss, names, packed = self._parse_root_scaled(losses, reduce=False)
            loss.backward(gradient=self._root_gradient(loss))
            cap.demb.copy_(g.grad[self.rank * B:(self.rank + 1) * B])
            if mlm is not None:
                cap.dmlm.copy_(mlm.grad)
            out.update(names=names, packed=packed, loss=loss.detach())

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # a pool of its own: it is captured after the backward graphs but replays BEFORE them — in the shared pool its
        # temporaries would land on blocks the backward capture released, i.e. on the activations the backward still reads
        gl = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gl, capture_error_mode='thread_local'):
            run()
        return gl, (g_static, out['names'], out['packed'], out['loss'])

    def optimizer_step(self):
        """Global-norm clip + AdamW on the slabs; no host synchronisation.  The clip coefficient, Adam's bias
        corrections and Adam's own step count live on the device (``clv_optim_prep``): a step with a non-finite
        gradient norm is skipped there and does not advance Adam's count (mmcv_Fp16OptimizerHook.py:123-141), while
        the LR index moves on like the reference's ``runner.iter``."""
        self._refuse_swapped('optimizer_step')
        lr = self.current_lr()
        self.lr_iter += 1
        self.step_count += 1
        if self.graph is None and not self._stale_cleared:
            # a caller's own loss.backward() (the style of an OptimizerHook) that did not go through finish_backward():
            # first-touch slots this backward did not reach still hold the previous step's gradient — clear them before
            # the norm.  With a reduced wire copy it is too late for that (the stale values have been exchanged).
            stale = self._stale_sinks()
            if stale:
                if self.wire is not None and self.reducer.active:
                    raise RuntimeError('first-touch gradient slots were not reached by this backward and the gradient '
                                       'exchange has already run: call engine.finish_backward() instead of '
                                       'engine.reducer.finish()')
                torch._foreach_zero_(stale)
        self._stale_cleared = False
        # DDP averages the summed gradients (the loss scale is divided out on the device); k virtual ranks are k more ranks
        gscale = 1.0 / (self.world * self.virtual_ranks)
        grads = self.wire if self.wire is not None else [seg.flat_g for seg in self.segments]   # reduced gradients
        fused = self._norm_tables is not None
        if fused and self._norm_state.dirty:   # a sink got a second gradient this step (ops.linear_wgrad): recompute it all
            if self.graph is not None:
                raise RuntimeError('fused gradient norm: a first-touch sink received two gradients inside a captured step; '
                                   'build the engine with CLOVER_FUSED_NORM=0')
            self._norm_state.dirty = False
            self.sumsq.zero_()
            fused = False
        if fused:                              # the first-touch slots' sums sit in the norm slots already
            for seg, (tab, nblk) in zip(self.segments, self._norm_tables):
                ops.sumsq_ranges(seg.flat_g, tab, nblk, self.sumsq)
        else:
            for g in grads:
                ops.sumsq_accumulate(g, self.sumsq)
        ops.optim_prep(self.sumsq, self.optim_state, self.betas[0], self.betas[1],
                       self.grad_clip if self.grad_clip else 0.0, gscale,
                       slots=self.sumsq[16:] if self._norm_tables is not None else None)
        if self._act is not None and self._overflow_report:
            # right behind the skip decision, where the gradient report goes: a skipped step keeps its forward records
            ops.act_report_latch(self.optim_state, self._act.live, self._act.latched, len(self._act.names))
        for seg, g in zip(self.segments, grads):
            ops.adamw_step_dev(seg.flat_p, g, seg.exp_avg, seg.exp_avg_sq, seg.shadow, self.optim_state,
                               lr * seg.lr_mult, self.betas[0], self.betas[1], self.eps, seg.weight_decay)
            seg.refresh_transposed()
        if self._overflow_report:              # behind the skip decision, ahead of the clearing: the evidence is still there
            for g, tab, out in zip(grads, self._grad_report_tables(), self._report_out):
                ops.grad_report(g, tab, self.optim_state, out, 0)
        self.zero_grads()
        self._act_end_step()
        self.last_lr = lr

    # ------------------------------------------------------------------ overflow report (csrc/grad_report.hip)
    def _grad_report_tables(self):
        """One clv_grad_report table per segment: every parameter's slab slot, phantom padding rows included (element
        offsets: the same table reads the fp32 slab and its 16-bit wire copy)."""
        if self._report_tables is None:
            def scanned(p):
                pad = getattr(p, '_clv_pad_grad', None)
                return pad.numel() if pad is not None else p.numel()
            self._report_tables = [ops.grad_report_table([(off, scanned(p)) for p, off in zip(sg.params, sg.offsets)],
                                                         self._device) for sg in self.segments]
        return self._report_tables

    def _report_rows(self, outs, offending_only):
        """Host side of a report (syncs): the segments' records as rows in TRUE gradient units."""
        reps = [ops.grad_report_read(out, tab) for out, tab in zip(outs, self._grad_report_tables())]
        head = reps[0]
        if head['n_params'] == 0:              # the kernels never wrote it
            return None
        scale = head['loss_scale'] if head['loss_scale'] > 0.0 else 1.0
        unit = 1.0 / (self.world * self.virtual_ranks) / scale
        rows = []
        for sg, rep in zip(self.segments, reps):
            for name, p, nf, mx, ss in zip(sg.names, sg.params, rep['nonfinite'].tolist(), rep['max_abs'].tolist(),
                                           rep['sumsq'].tolist()):
                if nf or not offending_only:
                    rows.append((name, p.numel(), int(nf), mx * unit, math.sqrt(ss) * unit))
        return dict(t=head['t'], skipped=head['skipped'], loss_scale=scale, rows=rows)

    def overflow_report(self):
        """What the last SKIPPED optimizer step found in its gradients (host sync) — ``None`` if this engine has not skipped
        a step yet, else ``dict(t, skipped, loss_scale, rows)``: Adam's step count and the count of skipped steps at that
        moment, the loss scale those gradients carried, and one row ``(name, numel, nonfinite, max_abs, norm)`` per
        parameter with a non-finite gradient element — ``max_abs`` and ``norm`` over the parameter's FINITE elements, in
        true gradient units (the loss scale and the 1 / (world * virtual_ranks) averaging divided out).  Steps that were
        taken leave it as it was.  Needs ``CloverEngine(..., overflow_report=True)``."""
        if not self._overflow_report:
            raise RuntimeError('overflow_report(): this engine was built without overflow_report=True, so its optimizer '
                               'steps do not take the report; pass CloverEngine(..., overflow_report=True) (tools/train.py: '
                               'the config key overflow_report = dict(interval=...))')
        rep = self._report_rows(self._report_out, offending_only=True)
        if rep is not None and self._act is not None:
            act = self._act
            rows = act.rows(ops.act_report_read(act.latched, len(act.names), latched=True), offending_only=True)
            rep['activations'] = dict(first=rows[0][0] if rows else None, rows=rows)
        return rep

    # ------------------------------------------------------------------ activation report (csrc/act_report.hip)
    @contextlib.contextmanager
    def _act_forward(self):
        """Around a forward pass the engine drives: the watched modules' hooks launch only in here."""
        act = self._act
        if act is None:
            yield
            return
        act.on = True
        try:
            yield
        finally:
            act.on = False

    def _act_begin_step(self):
        if self._act is not None:
            self._act.begin_step()

    def _act_end_step(self):
        if self._act is not None:
            self._act.stale = True

    def activation_stats(self):
        """The headroom view (host sync): ``dict(limit, rows)`` with one row ``(name, numel_per_call, calls, nonfinite,
        max_abs)`` per watched module, in forward order, from the live table as it stands — the forward passes of the last
        optimizer step (the table is cleared ahead of a step's first forward: an eager fill issued by the engine, not a node
        of the graphs).  ``max_abs`` is the largest finite magnitude the module's output held, ``limit`` the largest finite
        value of the build's 16-bit type (65504 in the fp16 build).  Needs ``CloverEngine(..., activation_report=True)``."""
        if self._act is None:
            raise RuntimeError('activation_stats(): this engine was built without activation_report=True, so its forward '
                               'passes do not scan their outputs; pass CloverEngine(..., activation_report=True) (tools/'
                               'train.py: the config key overflow_report = dict(interval=..., activations=True))')
        act = self._act
        rows = act.rows(ops.act_report_read(act.live, len(act.names), latched=False), offending_only=False)
        return dict(limit=float(torch.finfo(ops.BF16).max), rows=rows)

    def grad_stats(self):
        """The same rows for EVERY parameter of the gradients as they stand (host sync): call it between
        ``finish_backward()`` and ``optimizer_step()``.  ``loss_scale`` is the scale of the backward that just ran."""
        if self._stats_out is None:
            self._stats_out = [ops.grad_report_new(tab, self._device) for tab in self._grad_report_tables()]
        grads = self.wire if self.wire is not None else [seg.flat_g for seg in self.segments]
        for g, tab, out in zip(grads, self._grad_report_tables(), self._stats_out):
            ops.grad_report(g, tab, self.optim_state, out, 1)
        return self._report_rows(self._stats_out, offending_only=False)

    def step_stats(self):
        """What a log line wants of the optimizer's device record, in ONE read (host sync): ``loss_scale`` of the next
        backward (1.0 without a scaler), ``grad_norm`` of the last step (not finite when it was skipped), ``skipped`` and
        ``t`` (steps skipped / taken so far), ``skip`` (1: the last step was skipped), ``calls`` (optimizer_step() calls)."""
        st = ops.optim_state_read(self.optim_state)
        return dict(loss_scale=st['loss_scale'] if self._scaler_on else 1.0, grad_norm=st['norm'], skipped=st['skipped'],
                    t=st['t'], skip=st['skip'], calls=self.step_count)

    # ------------------------------------------------------------------ weight EMA (the reference's ema_hook)
    def ema_enable(self, skip_buffers=False):
        """Start keeping an exponential moving average of the weights (mmaction/core/hooks/ema.py:43-62).

        Every segment gets an fp32 slab ``ema`` laid out like ``flat_p`` and initialised to a copy of it (phantom padding
        rows included: zero, and they stay zero).  Every floating-point entry ``name`` of ``model.state_dict()`` is
        registered on the model as the buffer ``'ema_' + name.replace('.', '_')`` (the reference's naming, :55-59): a view
        into the ``ema`` slab for a slab parameter, a plain clone — a LOOSE entry of the kernels' table — for the rest:
        parameters the step never reaches (``unused_names``), frozen parameters and, unless ``skip_buffers``, float buffers
        such as BatchNorm1d's running statistics.  So ``state_dict()`` / checkpoints carry the average and
        ``load_state_dict`` writes into it in place; nothing else needs to know.  Integer and bool buffers
        (``num_batches_tracked``, index tables) take no part — the reference clones and swaps them without ever updating
        them, which exchanges equal values.  The average is fp32 over the fp32 masters whatever the 16-bit
        build; every rank of a data-parallel job keeps its own, identical, copy (no collective)."""
        if self._ema_table is not None:
            if bool(skip_buffers) != self._ema_skip_buffers:
                raise RuntimeError(f'ema_enable(skip_buffers={skip_buffers}): the EMA is already enabled with '
                                   f'skip_buffers={self._ema_skip_buffers}')
            return
        model = self.model
        param_names = {n for n, _ in model.named_parameters()}
        state = [(n, t) for n, t in model.state_dict(keep_vars=True).items() if t.dtype.is_floating_point]
        if skip_buffers:                       # :51-54 — only the parameters then
            state = [(n, t) for n, t in state if n in param_names]
        # by address, not by name: a tied tensor appears in state_dict() under every one of its names, and each memory
        # location may have only ONE entry in the table (one writer per element; a second entry would swap it back)
        slot = {q.data_ptr(): (sg, off) for sg in self.segments for q, off in zip(sg.params, sg.offsets)}
        entries, loose = [], {}
        for sg in self.segments:
            sg.ema = sg.flat_p.clone()
            entries.append((sg.flat_p, sg.ema, sg.shadow))
        for name, t in state:
            buf_name = 'ema_' + name.replace('.', '_')
            if t.data_ptr() in slot:
                sg, off = slot[t.data_ptr()]
                buf = sg.ema[off:off + t.numel()].view_as(t)
            elif t.data_ptr() in loose:
                buf = loose[t.data_ptr()]
            else:
                data = t.detach()
                if data.dtype != torch.float32 or not data.is_contiguous():
                    raise NotImplementedError(f'ema_enable: {name} ({data.dtype}, contiguous={data.is_contiguous()}) is '
                                              'outside the slabs and not a contiguous fp32 tensor')
                buf = loose[t.data_ptr()] = data.clone()
                entries.append((data, buf, None))
            model.register_buffer(buf_name, buf)
            self.ema_names[name] = buf_name
        self._ema_table = ops.ema_table(entries, self._device)
        self._ema_skip_buffers = bool(skip_buffers)

    def ema_update(self, momentum):
        """ema = (1 - momentum) * ema + momentum * weights for the whole model: one launch on the current stream, outside
        every graph (so ``momentum`` may change each call).  Once per optimizer step, also a skipped one."""
        if self._ema_table is None:
            raise RuntimeError('ema_update: call ema_enable() first')
        if self.ema_swapped:
            raise RuntimeError('ema_update while the EMA is swapped in: the parameters hold the average itself')
        ops.ema_update(self._ema_table, momentum)

    def ema_swap(self):
        """Exchange weights and average IN PLACE (every address a captured graph holds stays valid) and re-derive what
        the kernels compute from: the 16-bit shadows (written by the swap kernel with AdamW's rounding) and their W^T
        copies.  Toggles ``ema_swapped``; while it is set the training entry points refuse to run."""
        if self._ema_table is None:
            raise RuntimeError('ema_swap: call ema_enable() first')
        ops.ema_swap(self._ema_table)
        for sg in self.segments:
            sg.refresh_transposed()
        self.ema_swapped = not self.ema_swapped

    def _refuse_swapped(self, what):
        if self.ema_swapped:
            raise RuntimeError(f'CloverEngine.{what}() while the EMA weights are swapped in (ema_swapped): it would train '
                               'the averaged weights; call ema_swap() again first')

    def optimizer_state(self):
        """AdamW state for checkpoints: per segment the flat moments + names/offsets, and the step count."""
        st = ops.optim_state_read(self.optim_state)
        return dict(step=st['t'], skipped=st['skipped'], calls=self.step_count, lr_iter=self.lr_iter,
                    loss_scaler=self.loss_scaler_state(st),
                    segments=[dict(names=list(sg.names), offsets=list(sg.offsets), weight_decay=sg.weight_decay,
                                   lr_mult=sg.lr_mult,
                                   exp_avg=sg.exp_avg.detach().cpu(), exp_avg_sq=sg.exp_avg_sq.detach().cpu())
                              for sg in self.segments])

    def load_optimizer_state(self, state):
        self.step_count = int(state.get('calls', state['step']))
        self.lr_iter = int(state.get('lr_iter', state['step']))
        self.optim_state.zero_()
        self.optim_state[5] = int(state['step'])                 # Adam's t (ops.optim_state_read layout)
        self.optim_state[6] = int(state.get('skipped', 0))
        if self._scaler_on:
            sc = dict(cur_scale=self.scaler_cfg['init_scale'], cur_iter=0, last_overflow_iter=-1)
            if self.scaler_cfg['mode'] == 'dynamic':      # (a static scale is configuration, not state)
                sc.update(state.get('loss_scaler') or {})
            ops.optim_state_set_scaler(self.optim_state, sc['cur_scale'], self.scaler_cfg['mode'] == 'dynamic',
                                       self.scaler_cfg['scale_factor'], self.scaler_cfg['scale_window'],
                                       sc['cur_iter'], sc['last_overflow_iter'])
        assert len(self.segments) == len(state['segments']), 'optimizer state belongs to a different parameter layout'
        for sg, st in zip(self.segments, state['segments']):
            assert list(sg.names) == list(st['names']), 'optimizer state belongs to a different parameter layout'
            for key in ('weight_decay', 'lr_mult'):          # the slab's options are baked into its AdamW launch
                if key in st and abs(float(st[key]) - float(getattr(sg, key))) > 1e-12:
                    raise ValueError(f'optimizer state was saved with {key}={st[key]} for the slab of {sg.names[0]} ... '
                                     f'but the current paramwise_cfg gives {getattr(sg, key)}')
            if 'offsets' not in st or list(st['offsets']) == list(sg.offsets):
                sg.exp_avg.copy_(st['exp_avg'])
                sg.exp_avg_sq.copy_(st['exp_avg_sq'])
            else:
                # a checkpoint written under another slab layout (slot alignment / phantom padding rows changed between
                # rounds): same parameters, other offsets — re-scatter the moments per parameter by name instead of copying
                # the flat buffers (which would fail on the size, or silently misalign the moments)
                old_off = list(st['offsets'])
                sg.exp_avg.zero_()
                sg.exp_avg_sq.zero_()
                for i, (name, p_) in enumerate(zip(sg.names, sg.params)):
                    n = p_.numel()
                    if old_off[i] + n > st['exp_avg'].numel() or (i + 1 < len(old_off) and old_off[i + 1] - old_off[i] < n):
                        raise ValueError(f'optimizer state: the saved slot of {name} holds fewer than {n} elements '
                                         f'(checkpoint from a different model?)')
                    for dst, key in ((sg.exp_avg, 'exp_avg'), (sg.exp_avg_sq, 'exp_avg_sq')):
                        dst[sg.offsets[i]:sg.offsets[i] + n].copy_(st[key][old_off[i]:old_off[i] + n])
        self.refresh_shadow()

    def refresh_shadow(self):
        """Re-derive the bf16 compute copy from the fp32 slabs — after anything that writes parameters behind the
        optimizer's back (``load_state_dict`` of a checkpoint: it copies into the slab views in place)."""
        for sg in self.segments:
            sg.shadow.copy_(sg.flat_p)
            sg.refresh_transposed()

    @property
    def loss_scale(self):
        """The scale the NEXT backward will use (host sync; 1.0 without a scaler)."""
        return ops.optim_state_read(self.optim_state)['loss_scale'] if self._scaler_on else 1.0

    def loss_scaler_state(self, st=None):
        """LossScaler.state_dict() (fp16_utils.py:364-373) — what the reference keeps in runner.meta['fp16']['loss_scaler']
        (mmcv_Fp16OptimizerHook.py:147-149); None without a scaler."""
        if not self._scaler_on:
            return None
        st = st or ops.optim_state_read(self.optim_state)
        return dict(cur_scale=st['loss_scale'], cur_iter=st['scale_iter'], mode=self.scaler_cfg['mode'],
                    last_overflow_iter=st['last_overflow'], scale_factor=st['scale_factor'],
                    scale_window=st['scale_window'])

    def grad_norm(self):
        """Global gradient norm of the last step's (averaged) gradients — host sync, logging only."""
        return ops.optim_state_read(self.optim_state)['norm']

    def adam_steps(self):
        """Adam's own step count = optimizer steps actually taken (host sync)."""
        return ops.optim_state_read(self.optim_state)['t']
