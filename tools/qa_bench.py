#!/usr/bin/env python
"""Video-QA / fill-in-the-blank fine-tuning step at the reference's per-GPU shapes (Swin-B, 8 frames at 224^2, B = 16;
configs/finetune_{qa_mc,qa_oe,fib}_synthetic.py): one JSON line per task.

    python tools/qa_bench.py [--task mc oe fib] [--steps 20] [--warmup 5]

mc: 5 candidates x 100 tokens, QA_MC_head; oe: 40 tokens, 1540 answers; fib: 200 tokens, 908 answers, [MASK] row.
Each task: CloverEngine with the config's optimizer settings, one dry step, hipGraph capture, `warmup` replays, then
`steps` replays timed with events.  Reports clips/s, ms/step, the losses after the first step and the library-GEMM table
(empty: every GEMM of the step on the HIP kernels).  Synthetic batches (clover_amd/utils/qa_synthetic.py)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

TASKS = {'mc': ('finetune_qa_mc_synthetic.py', 100, dict(num_choices=5)),
         'oe': ('finetune_qa_oe_synthetic.py', 40, dict(num_labels=1540)),
         'fib': ('finetune_fib_synthetic.py', 200, dict(num_labels=908, fib=True))}


def run(task, steps, warmup, batch):
    import clover_amd
    from clover_amd import ops
    from clover_amd.engine import CloverEngine
    from clover_amd.runner import Config
    from clover_amd.utils.qa_synthetic import qa_batch
    name, tokens, qa = TASKS[task]
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', name))
    B = batch or cfg.videos_per_gpu
    torch.manual_seed(0)
    model = clover_amd.build_model(dict(cfg.model)).cuda().train()
    b = {k: v.cuda() for k, v in qa_batch(B, tokens, 8, 1234, **qa).items()}
    opt = cfg.optimizer
    eng = CloverEngine(model, b, lr=opt['base_lr'], betas=tuple(opt['betas']), eps=opt['eps'],
                       weight_decay=opt['weight_decay'], paramwise_cfg=opt['paramwise_cfg'],
                       grad_clip=cfg.optimizer_config['grad_clip']['max_norm'],
                       loss_scale=cfg.fp16['loss_scale'] if clover_amd._lib.HALF_F16 else None)
    ops.LIBRARY_GEMM_CALLS.clear()
    eng.dry_step(b)
    eng.capture(b)
    run_b = eng.input_buffers()
    first = eng.step(run_b)
    losses = {k: round(float(v), 5) for k, v in first['log_vars'].items()}
    for _ in range(warmup):
        eng.step(run_b)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        eng.step(run_b)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    return {'metric': f'video QA fine-tuning step ({task})', 'task': task, 'config': name, 'per_gpu_batch': B,
            'frames': 8, 'size': 224, 'tokens': tokens, **qa, 'hip_graph': True, 'steps': steps, 'warmup': warmup,
            'clips_per_s': round(B * 1000.0 / ms, 2), 'ms_per_step': round(ms, 3), 'losses_step1': losses,
            'dtype': 'f16' if clover_amd._lib.HALF_F16 else 'bf16',
            'library_gemm_calls': {f'{s}{list(sh)}': n for (s, sh), n in ops.LIBRARY_GEMM_CALLS.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--task', nargs='+', default=list(TASKS), choices=list(TASKS))
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--batch', type=int, default=None, help='videos per GPU (default: the config, 16)')
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/qa_bench.py needs an MI355X')
    for t in a.task:
        print(json.dumps(run(t, a.steps, a.warmup, a.batch)), flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
