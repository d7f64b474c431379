#!/usr/bin/env python
"""tools/train.py-style driver (reference: tools/train.py:26-88 arguments, :259-340 main, :101-256 train_model).

    python tools/train.py configs/pretrain_synthetic.py --launcher none --cfg-options total_epochs=1
    python -m torch.distributed.run --nproc-per-node 8 tools/train.py configs/pretrain_synthetic.py --launcher pytorch
    python tools/train.py configs/pretrain_overflow_report_synthetic.py --launcher none     # names what a skipped step overflowed in

Same config format (`_base_`, `model = dict(type='CloverPretrain', ...)`, `optimizer` with `base_lr`, `lr_config`,
`total_epochs`, `workflow`, `checkpoint_config`, `log_config`), same CLI names.  The dataset side (decoding,
tokenisation) is outside this project's scope: `data.synthetic` describes loaders of synthetic batches with the real
batch layout instead, and `data.packed = dict(path=..., train=dict(...), test=dict(...))` trains on pre-decoded uint8 clips
whose crop / resize / flip / normalise steps run on the device (clover_amd/utils/packed_loader.py, `ops.clip_prep`):

    python tools/pack_synthetic_clips.py work_dirs/packed_synthetic
    python tools/train.py configs/finetune_retrieval_packed_synthetic.py --launcher none --validate"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                            # noqa: E402
import torch.distributed as dist                        # noqa: E402


def parse_args():
    p = argparse.ArgumentParser(description='Train a recognizer')
    p.add_argument('config', help='train config file path')
    p.add_argument('--work_dir', help='the dir to save logs and models')
    p.add_argument('--resume-from', help='the checkpoint file to resume from')
    p.add_argument('--load-from', help='the checkpoint file to load from')
    p.add_argument('--validate', action='store_true',
                   help='whether to evaluate the checkpoint during training (cfg.evaluation over data.synthetic_test)')
    p.add_argument('--seed', type=int, default=None, help='random seed')
    p.add_argument('--cfg-options', nargs='+', default=[], help='a.b=c overrides merged into the config')
    p.add_argument('--launcher', choices=['none', 'pytorch'], default='pytorch', help='job launcher')
    return p.parse_args()


class SyntheticLoader:
    """`length` batches of synthetic pairs with the layout of the reference's collated batch."""

    def __init__(self, length, batch, frames, tokens, seed, device, qa=None):
        import bench
        from clover_amd.utils.qa_synthetic import qa_batch
        self.length = length

        def make(i):      # qa: dict(num_choices / num_labels / fib) of a video_qa / FIB config (utils.qa_synthetic)
            if qa is not None:
                return qa_batch(batch, tokens, frames, seed + i, **qa)
            return bench.synthetic_batch(batch, frames, tokens, seed + i)
        self.batches = [{k: v.to(device) for k, v in make(i).items()} for i in range(min(length, 4))]

    def __len__(self):
        return self.length

    def __iter__(self):
        for i in range(self.length):
            yield self.batches[i % len(self.batches)]


def engine_kwargs(cfg, lr, half_f16=True):
    """The CloverEngine arguments a config asks for (optimizer, grad clip, loss scaler, virtual_ranks)."""
    opt = cfg.optimizer
    return dict(lr=lr, betas=tuple(opt.get('betas', (0.9, 0.999))), eps=opt.get('eps', 1e-8),
                weight_decay=opt.get('weight_decay', 0.0), paramwise_cfg=opt.get('paramwise_cfg'),
                grad_clip=(cfg.get('optimizer_config', {}).get('grad_clip') or {}).get('max_norm', 0.0),
                # `fp16 = dict(loss_scale=...)` of a reference config (pretrain_webvid_cc3m.py:21) -> the engine's
                # device-resident loss scaler (fp16 build; the bf16 build keeps its default: none)
                loss_scale=(cfg.get('fp16') or {}).get('loss_scale') if half_f16 else None,
                # `virtual_ranks = k`: every optimizer step takes k batches whose contrastive losses see all k * B rows
                virtual_ranks=int(cfg.get('virtual_ranks', 1) or 1),
                # `overflow_report = dict(interval=...)`: skipped steps leave a per-parameter report (overflow_hook below)
                overflow_report=bool(cfg.get('overflow_report')),
                # `overflow_report = dict(..., activations=True, modules=[...])`: the forward outputs are scanned as well and
                # a skipped step names the first module whose output was non-finite (CloverEngine(activation_report=...))
                activation_report=activation_report_arg(cfg))


_ENGINE_KEYS = ('activations', 'modules')      # keys of `overflow_report` that configure the engine, not the hook


def activation_report_arg(cfg):
    """CloverEngine's ``activation_report`` from `overflow_report = dict(interval=..., activations=True, modules=[...])`:
    False without ``activations``; True, or dict(modules=[...]) when extra fnmatch patterns are listed."""
    spec = dict(cfg.get('overflow_report') or {})
    if spec.get('modules') and not spec.get('activations'):
        raise ValueError('overflow_report: `modules` lists extra modules for the activation report; set activations=True')
    if not spec.get('activations'):
        return False
    return dict(modules=list(spec['modules'])) if spec.get('modules') else True


def overflow_hook(cfg, rank=0):
    """The OverflowHook a config's top-level `overflow_report = dict(interval=..., top=..., max_consecutive_skips=...)` asks
    for, or None without the key.  Every rank gets one (a run of skipped steps must stop them all); rank 0 prints."""
    if not cfg.get('overflow_report'):
        return None
    from clover_amd.runner import OverflowHook
    hook_args = {k: v for k, v in dict(cfg.overflow_report).items() if k not in _ENGINE_KEYS}
    return OverflowHook(printer=print if rank == 0 else (lambda text: None), **hook_args)


def main():
    args = parse_args()
    from clover_amd.runner import (CheckpointHook, CloverRunner, Config, EvalHook, GroupedLoader, LogHook, LrUpdaterHook,
                                   parse_cfg_options, scaled_lr)
    import clover_amd
    from clover_amd.engine import CloverEngine

    cfg = Config.fromfile(args.config)
    cfg.merge_from_dict(parse_cfg_options(args.cfg_options))
    if args.work_dir is not None:
        cfg.work_dir = args.work_dir
    elif cfg.get('work_dir') is None:
        cfg.work_dir = os.path.join('./work_dirs', os.path.splitext(os.path.basename(args.config))[0])
    if not torch.cuda.is_available():
        raise SystemExit('tools/train.py needs an MI355X (no CPU fallback)')
    if args.launcher == 'none':
        rank, world = 0, 1
        torch.cuda.set_device(0)
    else:
        rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', 0)))
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        dist.init_process_group('nccl', rank=rank, world_size=world,
                                device_id=torch.device('cuda', torch.cuda.current_device()))
    dev = torch.device('cuda', torch.cuda.current_device())
    if args.seed is not None:
        torch.manual_seed(args.seed)
    else:
        torch.manual_seed(0)                             # identical init on every rank (== DDP broadcast)

    model = clover_amd.build_model(cfg.model.copy() if hasattr(cfg.model, 'copy') else dict(cfg.model)).to(dev)
    model.train()
    lr = scaled_lr(cfg, world)                           # tools/train.py:160-166
    packed = cfg.data.get('packed')
    if packed:                                           # uint8 clips from disk, prepared on the device (ops.clip_prep)
        from clover_amd.utils.packed_loader import packed_loaders
        loaders = packed_loaders(packed, 'train', cfg.get('videos_per_gpu', 1), dev, rank, world,
                                 seed=args.seed or 0)
    else:
        syn = cfg.data['synthetic']
        loaders = [SyntheticLoader(s['length'], cfg.get('videos_per_gpu', 1), s.get('frames', 8), s.get('tokens', 32),
                                   1000 * (i + 1) + rank, dev, qa=s.get('qa')) for i, s in enumerate(syn)]
    lrc = cfg.lr_config
    kw = engine_kwargs(cfg, lr, clover_amd._lib.HALF_F16)
    engine = CloverEngine(model, next(iter(loaders[0])), **kw)      # (virtual ranks: built and captured on ONE micro-batch)
    if lrc.get('policy', 'CosineAnnealing') != 'CosineAnnealing' or lrc.get('by_epoch', True):
        raise NotImplementedError('lr_config: only CosineAnnealing with by_epoch=False (the reference recipe)')
    if cfg.get('hip_graph', True):                       # static shapes: replay the step as hipGraphs
        first = next(iter(loaders[0]))
        engine.dry_step(first)                           # no optimizer step: training starts from the initial weights
        engine.capture(first)
        if packed and kw['virtual_ranks'] == 1:          # the clips go straight into the graphs' static `imgs` buffers
            for ld in loaders:                           # (k micro-batches per step cannot share one buffer)
                ld.engine = engine
    if kw['virtual_ranks'] > 1:                         # lists of k batches per step: runner.iter counts optimizer steps
        loaders = [GroupedLoader(ld, kw['virtual_ranks'], printer=print if rank == 0 else None) for ld in loaders]
    runner = CloverRunner(engine, model=model, work_dir=cfg.work_dir, max_epochs=cfg.total_epochs,
                          meta=dict(config_name=os.path.basename(args.config), seed=args.seed))
    # the LR follows runner.iter (batch indices), not the count of optimizer steps (two per index with two loaders)
    runner.register_hook(LrUpdaterHook(lr, **{k: v for k, v in dict(lrc).items() if k not in ('policy', 'by_epoch')}))
    if rank == 0:
        runner.register_hook(LogHook(cfg.get('log_config', {}).get('interval', 10), printer=print))
        if cfg.get('checkpoint_config'):
            runner.register_hook(CheckpointHook(cfg.work_dir, cfg.checkpoint_config.get('interval', 1)))
    if overflow_hook(cfg, rank) is not None:
        runner.register_hook(overflow_hook(cfg, rank))
    if args.validate:                                    # tools/train.py:192-209 — on EVERY rank: the collection is a collective
        from clover_amd.utils.synthetic_loaders import SyntheticTestLoader
        ev = dict(cfg.get('evaluation') or {})
        st = cfg.data.get('synthetic_test', dict(pairs=64, frames=8, tokens=32))
        qa = st.get('qa') if ev.get('test_fn') == 'use_itm_head_fn' else None
        embed = ev.get('test_fn') in (None, 'recall_for_video_text_retrieval')       # routed by the metrics, as EvalHook
        ev_metrics = [ev.get('metrics')] if isinstance(ev.get('metrics'), str) else list(ev.get('metrics') or [])
        mc = embed and 'video_qa_mc' in ev_metrics
        varied = embed and 'recall_for_video_text_retrieval_varied' in ev_metrics
        if packed and packed.get('test'):                # the packed test split through the centre-crop path
            from clover_amd.utils.packed_loader import packed_loaders
            val = packed_loaders(packed, 'test', cfg.get('videos_per_gpu', 8), dev, rank, world)[0]
        else:
            val = SyntheticTestLoader(st.get('pairs', 64), cfg.get('videos_per_gpu', 8), st.get('frames', 8),
                                      st.get('tokens', 32), rank, world, dev, qa=qa,
                                      candidates=st.get('candidates') if mc else None,
                                      captions=st.get('captions') if varied else None)
        runner.register_hook(EvalHook(val, printer=print if rank == 0 else None, **ev))
    if cfg.get('ema_hook'):                              # tools/train.py:212-220 — on EVERY rank: each keeps its own average
        from clover_amd.runner import EMA_HOOKS
        ema_cfg = dict(cfg.ema_hook)
        ema_type, priority = ema_cfg.pop('type'), ema_cfg.pop('priority', 49)
        if ema_type not in EMA_HOOKS:
            raise KeyError(f'ema_hook: type {ema_type!r} is not one of {sorted(EMA_HOOKS)}')
        if args.resume_from:
            # the checkpoint's ema_* entries (the raw weights, see BaseEMAHook) can only be loaded once the hook has
            # registered their buffers: the hook resumes again from its before_run
            ema_cfg.setdefault('resume_from', args.resume_from)
        # priority 49: ahead of CheckpointHook and EvalHook in after_train_epoch, so both see the averaged weights
        runner.register_hook(EMA_HOOKS[ema_type](**ema_cfg), priority=priority)
    if args.resume_from:
        runner.resume(args.resume_from)
    elif args.load_from:
        runner.load_checkpoint(args.load_from)
    runner.run(loaders, [tuple(w) for w in cfg.get('workflow', [('train', 1)])], cfg.total_epochs)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
