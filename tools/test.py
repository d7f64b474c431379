#!/usr/bin/env python
"""tools/test.py-style evaluation driver for the retrieval and video-QA tasks (reference: tools/test.py:27-100 arguments,
:130-260 main; collection mmaction/core/hooks/my_eval_hook.py:20-100; metrics video_dataset.py:189-195).

    python tools/test.py configs/finetune_retrieval_synthetic.py work_dirs/.../epoch_2.pth --eval recall_for_video_text_retrieval
    python -m torch.distributed.run --nproc-per-node 8 tools/test.py <config> <checkpoint> --launcher pytorch --eval ...

The model runs ``forward_test(separate_test=True)`` (the HIP Swin + BERT paths, forward only) over a test set sharded
rank-major; embeddings are collected over RCCL and rank 0 computes R@1/5/10, median rank.  The dataset side is out of
scope: ``data.synthetic_test`` describes a synthetic test set (``pairs`` random (clip, caption) pairs, so the metrics
of an untrained model sit at chance: R@K ~ 100 K / pairs).  A config with ``data.packed = dict(path=..., test=dict(...))``
(configs/finetune_retrieval_packed_synthetic.py) reads its test split from packed uint8 clips instead: centre crop, resize
and normalisation run on the device (``ops.clip_prep``, clover_amd/utils/packed_loader.py).

Zero-shot multiple choice (``evaluation = dict(metrics=['video_qa_mc'], test_fn='recall_for_video_text_retrieval')``, the
reference's finetune_msrvtt_mc.py; ``synthetic_test.candidates = C`` captions per video) and the many-caption protocol
(``recall_for_video_text_retrieval_varied`` in the config or after ``--eval``; ``synthetic_test.captions`` = counts per
video, ``--v2t`` adds the video -> text keys) run the same two encoders; their scores stay on the device
(ops.retrieval_group_best) and ``--out`` holds the chosen candidate per video as ``pred``.

Dual-softmax re-scoring (``--dual-softmax T``, or ``evaluation = dict(..., dual_softmax=T)`` in the config as
configs/finetune_retrieval_dsl_synthetic.py): the two recall metrics print ``DSL_Recall@K`` / ``DSL_MR`` next to the plain
keys (the prior runs over all queries of the test set), and with ``--topk K --out`` the file also holds ``dsl_topk``.

Video QA / fill-in-the-blank (a config with ``evaluation.test_fn='use_itm_head_fn'``, or ``--eval video_qa_mc`` /
``video_qa_oe``): ``forward_test`` scores every sample (multi_gpu_test_itm_finetune, my_eval_hook.py:317-380) and rank 0
prints ``acc`` / ``overall_acc`` (video_dataset.py:304-343) over ``data.synthetic_test`` = dict(pairs, frames, tokens,
qa=dict(num_choices / num_labels / fib)) samples."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                            # noqa: E402
import torch.distributed as dist                        # noqa: E402


def parse_args():
    p = argparse.ArgumentParser(description='test (and eval) a model')
    p.add_argument('config', help='test config file path')
    p.add_argument('checkpoint', help="checkpoint file ('none' = the seeded random init)")
    p.add_argument('--out', default=None, help='output result file (json)')
    p.add_argument('--eval', type=str, nargs='+', default=None,
                   help='evaluation metrics (default: recall_for_video_text_retrieval; video-QA configs: their '
                        'evaluation.metrics)')
    p.add_argument('--gpu-collect', action='store_true', help='accepted for CLI compatibility (collection is always RCCL)')
    p.add_argument('--topk', type=int, default=0,
                   help='retrieval only: score on the device and add the K best video indices per query to --out (1..16)')
    p.add_argument('--v2t', action='store_true',
                   help='recall_for_video_text_retrieval_varied only: add V2T_Recall@K / V2T_MR (best caption per video)')
    p.add_argument('--dual-softmax', type=float, default=None, metavar='T',
                   help='retrieval recall only: add the DSL_* keys, ranks under s * softmax(T * s) over all queries '
                        '(default: evaluation.dual_softmax of the config)')
    p.add_argument('--cfg-options', nargs='+', default=[], help='a.b=c overrides merged into the config')
    p.add_argument('--launcher', choices=['none', 'pytorch'], default='none', help='job launcher')
    return p.parse_args()


from clover_amd.utils.synthetic_loaders import SyntheticTestLoader      # noqa: E402,F401 (exported from here too)


def select_test(cfg, eval_metrics):
    """-> ('qa' | 'retrieval', metrics): the video-QA test loop when the config asks for it (evaluation.test_fn ==
    'use_itm_head_fn', as the reference's tools/test.py) or the --eval metrics are video-QA ones; retrieval otherwise,
    with the config's evaluation.metrics when --eval names none.  A config whose evaluation.test_fn is
    'recall_for_video_text_retrieval' (the reference's finetune_msrvtt_mc.py) keeps the embedding test loop whatever
    the metric: 'video_qa_mc' is then answered zero-shot from the retrieval embeddings."""
    from clover_amd.evaluation import QA_METRICS, RETRIEVAL_METRICS
    ev = cfg.get('evaluation') or {}
    cfg_metrics = [ev.get('metrics')] if isinstance(ev.get('metrics'), str) else list(ev.get('metrics') or [])
    embed = ev.get('test_fn') == 'recall_for_video_text_retrieval'
    qa = not embed and (ev.get('test_fn') == 'use_itm_head_fn' or any(m in QA_METRICS for m in (eval_metrics or [])))
    if not qa:
        metrics = eval_metrics or [m for m in cfg_metrics if m in RETRIEVAL_METRICS]
        return 'retrieval', metrics or ['recall_for_video_text_retrieval']
    metrics = eval_metrics or list(ev.get('metrics', ['video_qa_mc']))
    bad = [m for m in metrics if m not in QA_METRICS]
    if bad:
        raise SystemExit(f'--eval {bad}: a video-QA config evaluates {list(QA_METRICS)}')
    return 'qa', metrics


def main():
    args = parse_args()
    from clover_amd.runner import Config, parse_cfg_options
    from clover_amd.evaluation import (evaluate_qa, evaluate_retrieval, multi_gpu_test_itm_finetune,
                                       multi_gpu_test_retrieval, multi_gpu_test_retrieval_varied)
    import clover_amd
    cfg = Config.fromfile(args.config)
    cfg.merge_from_dict(parse_cfg_options(args.cfg_options))
    kind, metrics = select_test(cfg, args.eval)
    if args.topk and (kind != 'retrieval' or not 1 <= args.topk <= 16):
        raise SystemExit('--topk K: the retrieval test only, K in 1..16')
    mc = kind == 'retrieval' and 'video_qa_mc' in metrics
    varied = kind == 'retrieval' and 'recall_for_video_text_retrieval_varied' in metrics
    if args.v2t and not varied:
        raise SystemExit('--v2t: with recall_for_video_text_retrieval_varied only')
    dsl = args.dual_softmax if args.dual_softmax is not None else (cfg.get('evaluation') or {}).get('dual_softmax')
    if dsl is not None and (kind != 'retrieval' or mc or args.v2t):
        raise SystemExit('--dual-softmax: the two retrieval recall metrics only (not multiple choice, video QA or --v2t)')
    if not torch.cuda.is_available():
        raise SystemExit('tools/test.py needs an MI355X (no CPU fallback)')
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
    torch.manual_seed(0)
    model = clover_amd.build_model(cfg.model.copy() if hasattr(cfg.model, 'copy') else dict(cfg.model)).to(dev)
    if args.checkpoint != 'none':
        ckpt = torch.load(args.checkpoint, map_location='cpu')
        sd = ckpt.get('state_dict', ckpt)
        sd = {(k[7:] if k.startswith('module.') else k): v for k, v in sd.items()}
        res = model.load_state_dict(sd, strict=False)
        if rank == 0:
            print(f'loaded {args.checkpoint}: {len(res.missing_keys)} missing, {len(res.unexpected_keys)} unexpected keys')
    model.eval()
    st = cfg.data.get('synthetic_test', dict(pairs=64, frames=8, tokens=32))
    packed = cfg.data.get('packed')
    if packed and packed.get('test'):                     # uint8 clips from disk: centre crop + resize on the device
        from clover_amd.utils.packed_loader import packed_loaders
        loader = packed_loaders(packed, 'test', cfg.get('videos_per_gpu', 8), dev, rank, world)[0]
    else:
        loader = SyntheticTestLoader(st.get('pairs', 64), cfg.get('videos_per_gpu', 8), st.get('frames', 8),
                                     st.get('tokens', 32), rank, world, dev, qa=st.get('qa') if kind == 'qa' else None,
                                     candidates=st.get('candidates') if mc else None,
                                     captions=st.get('captions') if varied else None)
    on_device = bool(args.topk) or mc or varied           # scored on the device: only small integer vectors come back
    if kind == 'qa':
        results = multi_gpu_test_itm_finetune(model, loader)
    elif varied:
        results = multi_gpu_test_retrieval_varied(model, loader, to_host=False)
    else:
        results = multi_gpu_test_retrieval(model, loader, to_host=not on_device, with_label=mc)
    if rank == 0:
        if on_device:                                     # ranks, the K best videos per query, the chosen candidates
            metrics = evaluate_retrieval(results, metrics, topk=args.topk, with_pred=mc, v2t=args.v2t, dual_softmax=dsl)
        elif kind == 'qa':
            metrics = evaluate_qa(results, metrics)
        else:
            metrics = evaluate_retrieval(results, metrics, dual_softmax=dsl)
        topk, pred, dsl_topk = metrics.pop('topk', None), metrics.pop('pred', None), metrics.pop('dsl_topk', None)
        for k, v in metrics.items():
            print(f'{k}: {v:.04f}')                                                   # tools/test.py:255-256
        if args.out:
            out = dict(metrics={k: float(v) for k, v in metrics.items()}, pairs=int(len(results['index'])))
            if topk is not None:
                out['topk'] = topk.tolist()
            if dsl_topk is not None:
                out['dsl_topk'] = dsl_topk.tolist()
            if pred is not None:
                out['pred'] = pred.tolist()
            with open(args.out, 'w') as f:
                json.dump(out, f)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
