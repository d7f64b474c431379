"""Virtual ranks on the host: the loader grouping, the learning-rate rule, the config key on its way to the engine (a stub
stepper stands in for it: no GPU here), the exported loss-section symbols, and the engine's first refusal."""
import ctypes
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _tool(name):
    spec = importlib.util.spec_from_file_location(f'clv_tools_vr_{name}', os.path.join(ROOT, 'tools', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Loader:
    def __init__(self, n):
        self.items = [f'b{i}' for i in range(n)]

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def test_grouped_loader_lengths_remainder_and_order():
    from clover_amd.runner import GroupedLoader
    said = []
    g = GroupedLoader(_Loader(12), 4, printer=said.append)
    assert len(g) == 3 and not said
    assert list(g) == [['b0', 'b1', 'b2', 'b3'], ['b4', 'b5', 'b6', 'b7'], ['b8', 'b9', 'b10', 'b11']]
    assert list(g) == list(g)                                        # a fresh pass per epoch
    g = GroupedLoader(_Loader(11), 4, printer=said.append)
    assert len(g) == 2 and list(g) == [['b0', 'b1', 'b2', 'b3'], ['b4', 'b5', 'b6', 'b7']]
    assert len(said) == 1 and 'last 3 of 11' in said[0] and 'dropped' in said[0]
    g = GroupedLoader(_Loader(3), 4, printer=said.append)
    assert len(g) == 0 and list(g) == [] and len(said) == 2
    assert list(GroupedLoader(_Loader(2), 1, printer=None)) == [['b0'], ['b1']]
    with pytest.raises(ValueError):
        GroupedLoader(_Loader(2), 0)


def test_lr_scales_with_the_global_batch():
    from clover_amd.runner import Config, scaled_lr

    def cfg(**top):
        return Config(dict(dict(optimizer=dict(type='AdamW', base_lr=1e-6), videos_per_gpu=8), **top))
    assert scaled_lr(cfg(), 1) == pytest.approx(8e-6)
    assert scaled_lr(cfg(virtual_ranks=4), 1) == pytest.approx(32e-6)        # base_lr x videos_per_gpu x world x k
    assert scaled_lr(cfg(virtual_ranks=4), 2) == pytest.approx(64e-6)
    assert scaled_lr(cfg(virtual_ranks=1), 2) == pytest.approx(16e-6)
    c = cfg(virtual_ranks=4)
    scaled_lr(c, 1)
    assert 'base_lr' not in c.optimizer and c.optimizer['lr'] == pytest.approx(32e-6)
    fixed = Config(dict(optimizer=dict(type='AdamW', lr=3e-4), virtual_ranks=4))
    assert scaled_lr(fixed, 8) == 3e-4                                       # an explicit lr is nobody's to scale


class _Stepper:
    """Takes what tools/train.py hands the engine; one step() per optimizer step."""

    def __init__(self, model, sample_batch, **kw):
        self.model, self.sample, self.kw, self.seen = model, sample_batch, kw, []

    def step(self, batch):
        assert isinstance(batch, list) and len(batch) == self.kw['virtual_ranks']
        self.seen.append(list(batch))
        return dict(loss=torch.tensor(0.0), log_vars=dict(loss=0.0), num_samples=len(batch))


def test_config_key_reaches_the_stepper():
    from clover_amd.runner import CloverRunner, Config, GroupedLoader, scaled_lr
    train = _tool('train')
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'pretrain_virtual_ranks_synthetic.py'))
    base = Config.fromfile(os.path.join(ROOT, 'configs', 'pretrain_synthetic.py'))
    assert cfg.get('virtual_ranks') == 4 and base.get('virtual_ranks') is None
    lr, lr_base = scaled_lr(cfg, 1), scaled_lr(base, 1)
    assert lr == pytest.approx(4 * lr_base)
    kw = train.engine_kwargs(cfg, lr)
    assert kw['virtual_ranks'] == 4 and kw['lr'] == lr and kw['loss_scale'] == 'dynamic' and kw['grad_clip'] == 15
    assert train.engine_kwargs(base, lr_base)['virtual_ranks'] == 1
    assert train.engine_kwargs(cfg, lr, half_f16=False)['loss_scale'] is None
    lengths = [s['length'] for s in cfg.data['synthetic']]
    loaders = [GroupedLoader(_Loader(n), kw['virtual_ranks'], printer=None) for n in lengths]
    st = _Stepper(torch.nn.Linear(2, 2), 'b0', **kw)                  # built on ONE micro-batch
    runner = CloverRunner(st, work_dir=None, max_epochs=1)
    runner.run(loaders[:1], [('train', 1)], 1)
    assert runner.iter == lengths[0] // 4 == len(st.seen)             # runner.iter counts optimizer steps
    assert st.seen[0] == ['b0', 'b1', 'b2', 'b3'] and st.seen[-1][-1] == f'b{lengths[0] - 1}'


def test_large_loss_symbols_exported_by_both_builds():
    from clover_amd import _lib
    pkg = os.path.dirname(_lib.LIB_PATH)
    names = ['clv_infonce_large_min_g'] + [f'clv_{n}_{d}_large' for n in ('infonce', 'infonce_pair', 'normsoftmax')
                                           for d in ('fwd', 'bwd')]
    ts = set()
    for fname in ('libclover_hip_f16.so', 'libclover_hip.so'):
        so = ctypes.CDLL(os.path.join(pkg, fname))
        for name in names:
            assert hasattr(so, name) and name in _lib.SIGNATURES, (fname, name)
        ts.add(so.clv_infonce_large_min_g())
        # the per-row terms of the new path sit behind the old layout: 6 G (3 G) more floats
        wf = so.clv_infonce_work_floats
        wf.restype, wf.argtypes = ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32]
        assert wf(8, 16) == 12 * 8 * 16 + 4 * 8 + 9 * 64 + 6 * 8 + 16 + 6 * 8
    assert len(ts) == 1 and 64 <= ts.pop() <= 1024
    from clover_amd import ops
    assert ops.NCE_FORCE_LARGE is None


def test_engine_refuses_a_cpu_model_first():
    from clover_amd.engine import CloverEngine
    with pytest.raises(RuntimeError, match='no CPU path'):
        CloverEngine(torch.nn.Linear(2, 2), {}, virtual_ranks=4)
    with pytest.raises(TypeError):
        CloverEngine(torch.nn.Linear(2, 2), {}, virtual_rank=4)       # (the argument's name is part of the interface)
