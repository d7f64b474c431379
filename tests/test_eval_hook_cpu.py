"""runner.EvalHook on the host: schedule, rule inference and best-checkpoint keeping against the reference's rules
(mmaction/core/hooks/my_eval_hook.py:404-880), the new CLI flags and the exported retrieval symbols.  No GPU: a stub
stepper trains, a stub test_fn returns canned metrics per epoch."""
import ctypes
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Stepper:
    def __init__(self):
        self.model = torch.nn.Linear(2, 2)
        self.steps = 0

    def step(self, batch):
        self.steps += 1
        return dict(loss=torch.tensor(0.0), log_vars=dict(loss=0.0), num_samples=1)


def _run(tmp_path, canned, epochs, start_epoch=0, **hook_kw):
    """A run of `epochs` one-batch epochs with an EvalHook whose test_fn returns canned[call index] -> (runner, hook)."""
    from clover_amd.runner import CloverRunner, EvalHook
    st = _Stepper()
    runner = CloverRunner(st, work_dir=str(tmp_path / 'exp7'), max_epochs=epochs)
    runner.epoch = start_epoch
    calls = []

    def test_fn(model, loader):
        assert model is st.model and loader == ['val']
        calls.append(runner.epoch)
        return canned[len(calls) - 1] if isinstance(canned, list) else canned
    printed = []
    hook = EvalHook(['val'], test_fn=test_fn, printer=printed.append, **hook_kw)
    hook.printed = printed
    runner.register_hook(hook)
    runner.run([['b0']], [('train', 1)], epochs)
    return runner, hook


@pytest.mark.parametrize('kw,epochs,start_epoch,want', [
    (dict(interval=2), 6, 0, [2, 4, 6]),                               # every_n_epochs
    (dict(start=3, interval=2), 6, 0, [3, 5]),                         # ":660-661 epochs 3, 5, 7 if start==3 and interval==2"
    (dict(start=1, interval=3), 7, 0, [1, 4, 7]),
    (dict(start=5, interval=1), 3, 0, []),                             # start beyond the run
    (dict(start=0, interval=1), 2, 0, [1, 1, 2]),                      # runner.epoch >= start: once BEFORE the first epoch
    (dict(start=2, interval=1), 4, 2, [3, 3, 4]),                      # a resumed run (epoch 2) evaluates before training on
    (dict(start=2, interval=2), 5, 2, [4]),                            # ... unless the interval says no: (3 - 2) % 2
])
def test_schedule(tmp_path, kw, epochs, start_epoch, want):
    runner, hook = _run(tmp_path, {'Recall@1': 1.0}, epochs, start_epoch=start_epoch, save_best=None, **kw)
    assert [r['epoch'] for r in hook.records] == want
    assert all(r['mode'] == 'val' and r['Recall@1'] == 1.0 for r in hook.records)
    assert hook.printed == hook.records                                # printed through the printer, one line each
    assert 'hook_msgs' not in runner.meta and not os.path.exists(runner.work_dir)


def test_schedule_by_iter(tmp_path):
    from clover_amd.runner import CloverRunner, EvalHook
    st = _Stepper()
    runner = CloverRunner(st, work_dir=str(tmp_path), max_epochs=1)
    hook = EvalHook(['val'], test_fn=lambda m, l: {'acc': 0.5}, by_epoch=False, interval=2, save_best=None)
    runner.register_hook(hook)
    runner.run([['b0', 'b1', 'b2', 'b3', 'b4']], [('train', 1)], 1)
    assert [r['iter'] for r in hook.records] == [2, 4]


def test_rule_inference():
    from clover_amd.runner import EvalHook
    mk = lambda **kw: EvalHook([], test_fn=lambda m, l: {}, **kw)                       # noqa: E731
    assert mk(save_best='Recall@all').rule == 'greater'
    assert mk(save_best='acc').rule == 'greater' and mk(save_best='overall_acc').rule == 'greater'
    assert mk(save_best='qa_loss').rule == 'less' and mk(save_best='loss').rule == 'less'
    h = mk(save_best='auto')
    assert h.rule is None and h.key_indicator == 'auto'                # resolved at the first evaluation
    assert mk(save_best='MR', rule='less').rule == 'less'
    with pytest.raises(ValueError):
        mk(save_best='MR')                                             # unknown key without a rule
    with pytest.raises(KeyError):
        mk(save_best='acc', rule='bigger')
    with pytest.raises(ValueError):
        mk(interval=0)
    with pytest.raises(ValueError):
        mk(start=-1)
    with pytest.raises(KeyError):
        EvalHook([], test_fn='zeroshot_action_recognition')
    assert mk(save_best=None).save_best is None


def test_best_checkpoint_kept_and_resumed(tmp_path):
    from clover_amd.runner import CloverRunner, EvalHook
    canned = [{'Recall@1': v, 'MR': 9.0} for v in (10.0, 30.0, 20.0, 30.0, 40.0)]
    runner, hook = _run(tmp_path, canned, 5, save_best='auto')
    assert hook.key_indicator == 'Recall@1' and hook.rule == 'greater'         # 'auto': the first metric key
    wd = runner.work_dir
    # written on improvement only (epochs 1, 2, 5 — the tie at epoch 4 is no improvement); earlier best files are gone
    assert sorted(os.listdir(wd)) == ['exp7_best_Recall@1_epoch_5.pth']
    msgs = runner.meta['hook_msgs']
    assert msgs == dict(best_score=40.0, best_ckpt=os.path.join(wd, 'exp7_best_Recall@1_epoch_5.pth'))
    saves = [p for p in hook.printed if isinstance(p, str)]
    assert [s.split(' is saved as ')[1].split('.pth')[0] for s in saves] == [f'exp7_best_Recall@1_epoch_{e}' for e in (1, 2, 5)]
    ck = torch.load(msgs['best_ckpt'], map_location='cpu')
    assert ck['meta']['hook_msgs'] == msgs and ck['meta']['epoch'] == 5

    # resume: the best score so far carries over — a lower score writes nothing, a higher one replaces the file
    st = _Stepper()
    r2 = CloverRunner(st, work_dir=wd, max_epochs=7)
    r2.resume(msgs['best_ckpt'])
    assert r2.epoch == 5 and r2.meta['hook_msgs'] == msgs
    scores = iter([35.0, 50.0])
    h2 = EvalHook(['val'], test_fn=lambda m, l: {'Recall@1': next(scores)}, save_best='Recall@1')
    r2.register_hook(h2)
    r2.run([['b0']], [('train', 1)], 6)
    assert sorted(os.listdir(wd)) == ['exp7_best_Recall@1_epoch_5.pth'] and r2.meta['hook_msgs']['best_score'] == 40.0
    r2.run([['b0']], [('train', 1)], 7)
    assert sorted(os.listdir(wd)) == ['exp7_best_Recall@1_epoch_7.pth'] and r2.meta['hook_msgs']['best_score'] == 50.0

    # a 'less' key keeps the smallest
    runner, hook = _run(tmp_path / 'l', [{'qa_loss': v} for v in (3.0, 1.0, 2.0)], 3, save_best='qa_loss')
    assert sorted(os.listdir(runner.work_dir)) == ['exp7_best_qa_loss_epoch_2.pth']
    assert runner.meta['hook_msgs']['best_score'] == 1.0


def test_evaluation_restores_mode_and_checks_state(tmp_path):
    """The hook refuses a test loop that leaves the model in another mode than it found it."""
    from clover_amd.runner import CloverRunner, EvalHook
    st = _Stepper()
    runner = CloverRunner(st, work_dir=str(tmp_path), max_epochs=1)

    def bad(model, loader):
        model.eval()
        return {'acc': 1.0}
    runner.register_hook(EvalHook([], test_fn=bad, save_best=None))
    with pytest.raises(RuntimeError, match='disturbed'):
        runner.run([['b0']], [('train', 1)], 1)


def _tool(name):
    spec = importlib.util.spec_from_file_location(f'clv_tools_hook_{name}', os.path.join(ROOT, 'tools', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags_and_loader_export(monkeypatch):
    train, test = _tool('train'), _tool('test')
    monkeypatch.setattr(sys, 'argv', ['train.py', 'cfg.py', '--launcher', 'none'])
    assert train.parse_args().validate is False                                 # default off
    monkeypatch.setattr(sys, 'argv', ['train.py', 'cfg.py', '--validate', '--launcher', 'none'])
    assert train.parse_args().validate is True
    monkeypatch.setattr(sys, 'argv', ['test.py', 'cfg.py', 'ckpt.pth'])
    assert test.parse_args().topk == 0
    monkeypatch.setattr(sys, 'argv', ['test.py', 'cfg.py', 'ckpt.pth', '--topk', '5', '--out', 'o.json'])
    a = test.parse_args()
    assert (a.topk, a.out) == (5, 'o.json')
    from clover_amd.utils.synthetic_loaders import SyntheticTestLoader
    assert test.SyntheticTestLoader is SyntheticTestLoader
    ld = test.SyntheticTestLoader(pairs=5, batch=2, frames=2, tokens=8, rank=1, world=2, device='cpu')
    assert [b['index'].tolist() for b in ld] == [[1, 3]] and len(ld) == 1


def test_retrieval_symbols_exported_by_both_builds():
    from clover_amd import _lib
    assert _lib.ABI_VERSION == 20
    pkg = os.path.dirname(_lib.LIB_PATH)
    for fname in ('libclover_hip_f16.so', 'libclover_hip.so'):
        so = ctypes.CDLL(os.path.join(pkg, fname))
        assert so.clv_abi_version() == 20, fname
        for name in ('clv_retrieval_work_bytes', 'clv_retrieval_rank'):
            assert hasattr(so, name) and name in _lib.SIGNATURES, (fname, name)
        wb = so.clv_retrieval_work_bytes
        wb.restype, wb.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
        assert wb(1000, 1000, 768, 0) == 2000 * 768 * 4                         # the two normalised operands, nothing else
        assert wb(8, 8, 6, 0) == -2 and wb(8, 8, 8, 17) == -2 and wb(0, 8, 8, 0) == -2 and wb(8, 8, 4100, 0) == -2
    from clover_amd import ops
    from clover_amd.evaluation import recall_on_device                           # noqa: F401
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_rank(torch.zeros(2, 4), torch.zeros(2, 4))
