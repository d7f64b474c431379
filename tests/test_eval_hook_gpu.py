"""runner.EvalHook on the GPU: the evaluation sees the weights the engine trains, leaves the training untouched, and
`tools/train.py --validate` / `tools/test.py --topk` end to end.  `-m gpu` only."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import closed_form as cf
from test_engine_gpu import batch, make_finetune_model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_KEYS = ('imgs', 'token_ids', 'segment_ids', 'input_mask')


def rel(a, b):
    a, b = a.detach().double().cpu().numpy().reshape(-1), b.detach().double().cpu().numpy().reshape(-1)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-20)


def val_loader(n=3, B=2):
    """n test batches of B pairs with `index`, as the reference's test pipeline emits."""
    out = []
    for i in range(n):
        b = {k: v.to(DEV) for k, v in cf.cf_batch(B, tag=f'val{i}').items() if k in TEST_KEYS}
        b['index'] = torch.arange(i * B, (i + 1) * B, device=DEV)
        out.append(b)
    return out


def test_current_weights_are_evaluated(tmp_path):
    """After 3 engine steps the hook's retrieval loop, run on the engine-bound model, must embed with the TRAINED weights:
    a fresh model (no engine) loaded from the checkpoint written at that moment agrees at the tolerance of
    test_forward_test_embeddings (2e-2) with equal metrics; a fresh model with the INITIAL weights does not (which is what
    a stale 16-bit shadow would compute)."""
    from clover_amd.engine import CloverEngine
    from clover_amd.evaluation import evaluate_retrieval, multi_gpu_test_retrieval
    from clover_amd.runner import CloverRunner, EvalHook
    b, loader = batch(4, 'evalw'), val_loader()
    m = make_finetune_model()
    eng = CloverEngine(m, b, lr=1e-3, weight_decay=0.0, grad_clip=15.0, max_iters=10 ** 9)
    for _ in range(3):
        eng.step(b)
    runner = CloverRunner(eng, model=m, work_dir=str(tmp_path), max_epochs=1)
    hook = EvalHook(loader, save_best=None)
    hook.after_train_epoch(runner)
    assert len(hook.records) == 1 and hook.records[0]['epoch'] == 1
    got = multi_gpu_test_retrieval(m, loader, to_host=False)
    assert got['video_embd'].is_cuda and got['video_embd'].shape == (6, 128) and got['index'].tolist() == list(range(6))
    assert {k: v for k, v in hook.records[0].items() if k not in ('epoch', 'mode')} == evaluate_retrieval(got)
    host = multi_gpu_test_retrieval(m, loader)                          # the default still returns numpy arrays
    assert isinstance(host['video_embd'], np.ndarray) and np.array_equal(host['video_embd'], got['video_embd'].cpu().numpy())
    path = runner.save_checkpoint(str(tmp_path), 'now.pth')

    m2 = make_finetune_model()
    m2.load_state_dict(torch.load(path, map_location='cpu')['state_dict'], strict=False)
    ref = multi_gpu_test_retrieval(m2, loader, to_host=False)
    m3 = make_finetune_model()                                          # the initial weights
    old = multi_gpu_test_retrieval(m3, loader, to_host=False)
    for k in ('video_embd', 'text_embd'):
        print(k, 'trained vs checkpoint', rel(got[k], ref[k]), 'initial vs checkpoint', rel(old[k], ref[k]))
    for k in ('video_embd', 'text_embd'):
        assert rel(got[k], ref[k]) < 2e-2
        assert rel(old[k], ref[k]) > 2e-2
    assert evaluate_retrieval(got) == evaluate_retrieval(ref)


def test_training_is_undisturbed(tmp_path):
    """Two engines from the same init, same seeds, hipGraph mode, two epochs of two batches — one with
    EvalHook(interval=1).  Epoch 2's logged losses agree within 2e-2 max(1, |loss|) (the bound
    test_checkpoint_roundtrip_through_engine uses for "same weights -> same loss"; fp32 atomics in the norm gradients rule
    out bit equality), the model is back in train mode and no graph set was added or dropped."""
    from clover_amd import ops
    from clover_amd.engine import CloverEngine
    from clover_amd.runner import CloverRunner, EvalHook, LogHook
    bs = [batch(2, f'und{i}') for i in range(2)]
    loader = val_loader()

    def run(with_hook):
        torch.manual_seed(11)
        ops._dropout_counter(DEV).fill_(20240611)          # both runs draw the same dropout masks — unless the evaluation
        m = make_finetune_model().train()                  # advanced the counter between them
        eng = CloverEngine(m, bs[0], lr=2e-4, weight_decay=0.0, grad_clip=15.0, max_iters=10 ** 9)
        eng.dry_step(bs[0])
        assert eng.capture(bs[0])
        runner = CloverRunner(eng, model=m, work_dir=str(tmp_path / f'h{int(with_hook)}'), max_epochs=2)
        log = LogHook(interval=1)
        runner.register_hook(log)
        hook = None
        if with_hook:
            hook = EvalHook(loader, interval=1, save_best='Recall@all')
            runner.register_hook(hook)
        runner.run([bs], [('train', 1)], 2)
        torch.cuda.synchronize()
        assert m.training and len(eng._captures) == 1
        return [r['loss'] for r in log.records], hook, runner

    plain, _, _ = run(False)
    hooked, hook, runner = run(True)
    print('losses without hook', plain, 'with hook', hooked)
    assert len(plain) == len(hooked) == 4
    for a, h in zip(plain[2:], hooked[2:]):
        assert abs(a - h) <= 2e-2 * max(1.0, abs(a)), (plain, hooked)
    assert [r['epoch'] for r in hook.records] == [1, 2]
    best = max(hook.records, key=lambda r: (r['Recall@all'], -r['epoch']))
    files = os.listdir(runner.work_dir)
    assert files == [f'h1_best_Recall@all_epoch_{best["epoch"]}.pth'], files
    assert runner.meta['hook_msgs']['best_score'] == best['Recall@all']


def _best_checkpoint(wd, stdout, key):
    """One metrics line per epoch; exactly one *_best_* file, named after the best epoch printed, whose meta carries the
    best logged value."""
    recs = [eval(ln) for ln in stdout.splitlines() if ln.startswith('{') and "'mode': 'val'" in ln]     # printed dicts
    assert [r['epoch'] for r in recs] == [1, 2], stdout[-3000:]
    best = max(recs, key=lambda r: (r[key], -r['epoch']))          # the first epoch to reach the best value keeps the file
    files = [f for f in os.listdir(wd) if '_best_' in f]
    assert files == [f'{os.path.basename(str(wd))}_best_{key}_epoch_{best["epoch"]}.pth'], (files, recs)
    ck = torch.load(os.path.join(str(wd), files[0]), map_location='cpu')
    assert ck['meta']['hook_msgs']['best_score'] == best[key]
    assert os.path.basename(ck['meta']['hook_msgs']['best_ckpt']) == files[0] and ck['meta']['epoch'] == best['epoch']
    return recs


@pytest.mark.parametrize('name', ['retrieval', 'qa_mc'])
def test_tools_train_validate(name, tmp_path):
    """tools/train.py --validate on a synthetic config in a child process, two short epochs."""
    cfg = os.path.join(ROOT, 'configs', f'finetune_{name}_synthetic.py')
    wd = tmp_path / 'work'
    qa = ", 'qa': {'num_choices': 5}" if name == 'qa_mc' else ''
    tokens = 100 if name == 'qa_mc' else 32
    opts = ['videos_per_gpu=2', "log_config={'interval': 1}",
            f"data.synthetic=[{{'length': 2, 'frames': 8, 'tokens': {tokens}{qa}}}]",
            f"data.synthetic_test={{'pairs': 6, 'frames': 8, 'tokens': {tokens}{qa}}}"]
    base = [sys.executable, os.path.join(ROOT, 'tools', 'train.py'), cfg, '--launcher', 'none', '--work_dir', str(wd),
            '--validate', '--cfg-options', *opts]
    r = subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    key = 'Recall@1' if name == 'retrieval' else 'acc'             # save_best='auto': the first metric key
    recs = _best_checkpoint(wd, r.stdout, key)
    assert all(np.isfinite(v) for rec in recs for v in rec.values() if not isinstance(v, str))
    assert len([ln for ln in r.stdout.splitlines() if "'mode': 'val'" not in ln and ln.startswith("{'epoch'")]) == 4


def test_tools_test_topk(tmp_path):
    cfg = os.path.join(ROOT, 'configs', 'finetune_retrieval_synthetic.py')
    out = tmp_path / 'res.json'
    opts = ['videos_per_gpu=4', "data.synthetic_test={'pairs': 10, 'frames': 8, 'tokens': 32}"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), cfg, 'none', '--topk', '5', '--out', str(out),
                        '--cfg-options', *opts], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert re.search(r'^Recall@1: \d', r.stdout, re.M) and 'topk' not in r.stdout
    res = json.load(open(out))
    topk = np.array(res['topk'])
    assert res['pairs'] == 10 and topk.shape == (10, 5) and set(res['metrics']) == {'Recall@1', 'Recall@5', 'Recall@10',
                                                                                    'MR', 'Recall@all'}
    assert topk.min() >= 0 and topk.max() < 10 and all(len(set(row)) == 5 for row in topk.tolist())
