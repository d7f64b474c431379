"""The weight-EMA hooks on the host: momentum schedules, call schedule, hook ordering and buffer names (no GPU)."""
import inspect
import math

import pytest
import torch

from clover_amd.runner import (BaseEMAHook, CheckpointHook, CloverRunner, EvalHook, ExpMomentumEMAHook, Hook,
                               LinearMomentumEMAHook)


# ---------------------------------------------------------------------------------------------- 1. momentum schedules
XS = (0, 1, 99, 1999, 10 ** 5)


@pytest.mark.parametrize('interval', [1, 4])
def test_momentum_schedules(interval):
    """Both schedules against their formulas, restated here: exponential  (1 - m) exp(-(1 + x) / T) + m,
    linear  min(m ** interval, (1 + x) / (W + x))."""
    for m, T in ((0.0002, 2000), (0.01, 20), (0.3, 7)):
        h = ExpMomentumEMAHook(momentum=m, interval=interval, total_iter=T)
        for x in XS:
            want = (1.0 - m) * math.exp(-(1.0 + x) / T) + m
            assert h.momentum_fun(x) == pytest.approx(want, rel=1e-15, abs=0.0), (m, T, x)
            assert m <= h.momentum_fun(x) <= 1.0
    for m, W in ((0.0002, 100), (0.5, 3), (0.9, 1000)):
        h = LinearMomentumEMAHook(momentum=m, interval=interval, warm_up=W)
        for x in XS:
            want = min(m ** interval, (1.0 + x) / (W + x))
            assert h.momentum_fun(x) == pytest.approx(want, rel=1e-15, abs=0.0), (m, W, x)
    # the cap of the linear schedule is what decides early on, the power later
    h = LinearMomentumEMAHook(momentum=0.9, interval=interval, warm_up=1000)
    assert h.momentum_fun(0) == 1 / 1000 and h.momentum_fun(10 ** 5) == 0.9 ** interval
    # get_momentum reads runner.iter; the base class without a function returns the constant

    class R:
        iter = 99
    assert ExpMomentumEMAHook(momentum=0.01, total_iter=20).get_momentum(R) == (1 - 0.01) * math.exp(-100 / 20) + 0.01
    assert BaseEMAHook(momentum=0.25).get_momentum(R) == 0.25
    assert BaseEMAHook(momentum=0.25, momentum_fun=lambda x: x / 1000).get_momentum(R) == 0.099


def test_constructor_defaults_and_refusals():
    def defaults(cls):
        return {k: p.default for k, p in inspect.signature(cls.__init__).parameters.items()
                if p.default is not inspect.Parameter.empty}
    assert defaults(BaseEMAHook) == dict(momentum=0.0002, interval=1, skip_buffers=False, resume_from=None,
                                         momentum_fun=None)
    assert defaults(ExpMomentumEMAHook) == dict(total_iter=2000)
    assert defaults(LinearMomentumEMAHook) == dict(warm_up=100)
    for cls in (ExpMomentumEMAHook, LinearMomentumEMAHook):
        h = cls()
        assert (h.momentum, h.interval, h.skip_buffers, h.checkpoint) == (0.0002, 1, False, None)
        h = cls(momentum=0.1, interval=3, skip_buffers=True, resume_from='x.pth')
        assert (h.momentum, h.interval, h.skip_buffers, h.checkpoint) == (0.1, 3, True, 'x.pth')
    for cls in (BaseEMAHook, ExpMomentumEMAHook, LinearMomentumEMAHook):
        for bad in (0, 1, 0.0, 1.0, -0.1, 1.5):
            with pytest.raises(AssertionError):
                cls(momentum=bad)


# ---------------------------------------------------------------------------------------------- 2. call schedule
class FakeEngine:
    """Records what the hook asks of the engine, with the runner's position at that moment."""

    def __init__(self):
        self.log, self.runner, self.ema_swapped, self.ema_names = [], None, False, {}

    def _at(self):
        return (self.runner.epoch, self.runner.iter)

    def step(self, batch):
        assert not self.ema_swapped, 'a training step while the EMA is swapped in'
        self.log.append(('step', batch) + self._at())
        return dict(loss=torch.zeros(()), log_vars={}, num_samples=1)

    def ema_enable(self, skip_buffers=False):
        self.log.append(('enable', skip_buffers))

    def ema_update(self, momentum):
        self.log.append(('update', momentum) + self._at())

    def ema_swap(self):
        self.ema_swapped = not self.ema_swapped
        self.log.append(('swap', self.ema_swapped) + self._at())


def fake_runner(**kw):
    eng = FakeEngine()
    runner = CloverRunner(eng, model=torch.nn.Linear(2, 2), max_epochs=kw.pop('max_epochs', 2), **kw)
    eng.runner = runner
    return eng, runner


@pytest.mark.parametrize('interval', [1, 4])
def test_call_schedule_single_loader(interval):
    eng, runner = fake_runner()
    hook = LinearMomentumEMAHook(momentum=0.5, interval=interval, warm_up=3, skip_buffers=True)
    runner.register_hook(hook, priority=49)
    runner.run([list(range(6))], [('train', 1)], 2)
    assert eng.log[0] == ('enable', True)
    updates = [e for e in eng.log if e[0] == 'update']
    want_iters = [it for it in range(12) if (it + 1) % interval == 0]
    assert [e[3] for e in updates] == want_iters
    for e in updates:                                  # the momentum of THAT iteration
        assert e[1] == min(0.5 ** interval, (1 + e[3]) / (3 + e[3]))
    # an update follows its own step
    for e in updates:
        assert eng.log[eng.log.index(e) - 1][0] == 'step' and eng.log[eng.log.index(e) - 1][3] == e[3]
    # swaps: out at the start of every epoch (the first one included), in at its end
    swaps = [e for e in eng.log if e[0] == 'swap']
    assert swaps == [('swap', False, 0, 0), ('swap', True, 0, 6), ('swap', False, 1, 6), ('swap', True, 1, 12)]
    # ... which brackets every epoch's steps
    kinds = [e[0] for e in eng.log if e[0] in ('swap', 'step')]
    assert kinds == ['swap'] + ['step'] * 6 + ['swap'] + ['swap'] + ['step'] * 6 + ['swap']


def test_call_schedule_two_loaders():
    """clover_runner.py:76-91 — both loaders' steps of one batch index share runner.iter; the hook updates after each."""
    eng, runner = fake_runner(max_epochs=1)
    runner.register_hook(ExpMomentumEMAHook(momentum=0.01, total_iter=20, interval=2), priority=49)
    runner.run([['a0', 'a1', 'a2', 'a3'], ['b0', 'b1', 'b2', 'b3']], [('train', 1)], 1)
    steps = [e for e in eng.log if e[0] == 'step']
    updates = [e for e in eng.log if e[0] == 'update']
    assert len(steps) == 8 and [e[3] for e in steps] == [0, 0, 1, 1, 2, 2, 3, 3]
    assert [e[3] for e in updates] == [1, 1, 3, 3]                        # one per loader step where (iter + 1) % 2 == 0
    assert all(e[1] == (1 - 0.01) * math.exp(-(1 + e[3]) / 20) + 0.01 for e in updates)
    eng1, runner1 = fake_runner(max_epochs=1)
    runner1.register_hook(ExpMomentumEMAHook(), priority=49)
    runner1.run([['a0', 'a1'], ['b0', 'b1']], [('train', 1)], 1)
    assert len([e for e in eng1.log if e[0] == 'update']) == len([e for e in eng1.log if e[0] == 'step']) == 4


class Tracer(Hook):
    def __init__(self, name, trace):
        self.name, self.trace = name, trace

    def after_train_epoch(self, runner):
        self.trace.append(self.name)


def test_priority_49_runs_before_checkpoint_and_eval_registered_earlier(tmp_path):
    eng, runner = fake_runner(max_epochs=1, work_dir=str(tmp_path))
    order = []

    class Ckpt(CheckpointHook):
        def after_train_epoch(self, r):
            order.append(('ckpt', r.stepper.ema_swapped))

    class Eval(EvalHook):
        def after_train_epoch(self, r):
            order.append(('eval', r.stepper.ema_swapped))

    class Ema(ExpMomentumEMAHook):
        def after_train_epoch(self, r):
            super().after_train_epoch(r)
            order.append(('ema', r.stepper.ema_swapped))

    runner.register_hook(Ckpt(str(tmp_path)))
    runner.register_hook(Eval([], save_best=None))
    runner.register_hook(Ema(), priority=49)
    assert [type(h).__name__ for h in runner.hooks] == ['Ema', 'Ckpt', 'Eval']
    runner.run([[0, 1]], [('train', 1)], 1)
    assert order == [('ema', True), ('ckpt', True), ('eval', True)]


def test_hooks_without_priority_keep_registration_order():
    _, runner = fake_runner()
    trace = []
    names = ['a', 'b', 'c', 'd', 'e']
    for n in names:
        runner.register_hook(Tracer(n, trace))
    assert [h.name for h in runner.hooks] == names
    runner.register_hook(Tracer('late60', trace), priority=60)
    runner.register_hook(Tracer('early49', trace), priority=49)
    runner.register_hook(Tracer('f', trace))                      # 50: behind the other 50s, ahead of 60
    runner.register_hook(Tracer('early49b', trace), priority=49)   # equal priorities: registration order
    runner.register_hook(Tracer('low', trace), priority='LOW')
    runner.register_hook(Tracer('first', trace), priority='HIGHEST')
    want = ['first', 'early49', 'early49b'] + names + ['f', 'late60', 'low']
    assert [h.name for h in runner.hooks] == want
    runner.call_hook('after_train_epoch')
    assert trace == want
    with pytest.raises(ValueError):
        runner.register_hook(Tracer('x', trace), priority=101)


def test_non_engine_stepper_is_refused():
    class Module(torch.nn.Linear):
        def train_step(self, batch, optimizer):
            return dict(loss=torch.zeros(()), log_vars={}, num_samples=1)

    m = Module(2, 2)
    runner = CloverRunner(m, model=m, max_epochs=1)
    runner.register_hook(ExpMomentumEMAHook(), priority=49)
    with pytest.raises(TypeError, match='CloverEngine'):
        runner.run([[0]], [('train', 1)], 1)
    assert not any(n.startswith('ema_') for n, _ in m.named_buffers())


def test_resume_follows_enable(tmp_path):
    """before_run: the buffers are registered first, then the checkpoint is loaded (so its ema_* entries find them)."""
    eng, runner = fake_runner(max_epochs=1)
    calls = []
    eng.ema_enable = lambda skip_buffers=False: calls.append('enable')
    runner.resume = lambda path: calls.append(('resume', path))
    ExpMomentumEMAHook(resume_from='ck.pth').before_run(runner)
    assert calls == ['enable', ('resume', 'ck.pth')]


# ---------------------------------------------------------------------------------------------- 3. buffer names
def test_buffer_names_follow_the_reference_rule():
    """'ema_' + the state_dict name with dots turned into underscores; registered through the engine's own ema_enable, run
    here on a stand-in for the engine's attributes with a model on the host (every entry is then a loose one, and the
    kernels' table is not built)."""
    from clover_amd import engine as E, ops

    class Inner(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(3, 2)
            self.bn = torch.nn.BatchNorm1d(2)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = torch.nn.ModuleList([Inner(), Inner()])
            self.head_w = torch.nn.Parameter(torch.ones(2))
            self.register_buffer('steps', torch.zeros((), dtype=torch.long))

    for skip in (False, True):
        net = Net()
        before = dict(net.state_dict())
        eng = E.CloverEngine.__new__(E.CloverEngine)
        eng.model, eng.segments, eng._device = net, [], torch.device('cpu')
        eng._ema_table, eng.ema_names, eng.ema_swapped = None, {}, False
        real, ops.ema_table = ops.ema_table, lambda entries, device: ('table', len(entries))
        try:
            eng.ema_enable(skip_buffers=skip)
        finally:
            ops.ema_table = real
        floating = [n for n, t in before.items() if t.dtype.is_floating_point]
        params = [n for n, _ in net.named_parameters()]
        want = params if skip else floating
        assert set(eng.ema_names) == set(want)
        assert eng._ema_table == ('table', len(want))
        for n in want:
            assert eng.ema_names[n] == 'ema_' + n.replace('.', '_')
            buf = dict(net.named_buffers())[eng.ema_names[n]]
            assert torch.equal(buf, before[n]) and buf.data_ptr() != before[n].data_ptr()
        assert eng.ema_names['backbone.1.fc.weight'] == 'ema_backbone_1_fc_weight'
        # integer buffers take no part, and the state_dict now carries the average
        sd = net.state_dict()
        assert 'ema_steps' not in sd and 'ema_backbone_0_bn_num_batches_tracked' not in sd
        assert ('ema_backbone_0_bn_running_mean' in sd) == (not skip)
        assert set(sd) == set(before) | {eng.ema_names[n] for n in want}
