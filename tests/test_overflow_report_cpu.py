"""The overflow report on the host: the table builder's chunking, OverflowHook against a fake stepper, the tools/train.py
config key, and the header's prototype against the ctypes binding (no GPU)."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

from clover_amd.runner import CloverRunner, Config, LogHook, OverflowHook

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 1. the table
def test_table_chunking():
    """Every parameter is cut into chunks of <= SUMSQ_CHUNK elements that cover it exactly once, in order and adjacent in
    the chunk list; an empty parameter has a record and no chunk; offsets are carried through."""
    from clover_amd import ops
    C = ops.SUMSQ_CHUNK
    assert C == 16384
    sizes = [1, 0, 7, C - 1, C, C + 1, 0, 2 * C, 2 * C + 1, 40000, 0]
    offs, pos = [], 24                                     # the buffer need not start with the first parameter
    for n in sizes:
        offs.append(pos)
        pos += (n + 7) // 8 * 8 + 8                        # 8-aligned slots with a gap between them
    prows, crows = ops.grad_report_chunks(list(zip(offs, sizes)))
    assert len(prows) == len(sizes)
    assert [n for _, n in prows] == [0 if n == 0 else (n + C - 1) // C for n in sizes]
    assert [n for _, n in prows] == [1, 0, 1, 1, 1, 2, 0, 2, 3, 3, 0]
    covered = torch.zeros(pos, dtype=torch.int32)
    nxt = 0
    for i, ((first, cnt), off, n) in enumerate(zip(prows, offs, sizes)):
        assert first == nxt                                # adjacent, in parameter order
        nxt += cnt
        at = off
        for p, start, count in crows[first:first + cnt]:
            assert p == i and start == at and 1 <= count <= C
            assert (start - off) % C == 0                  # an 8-aligned parameter keeps every chunk 16-byte aligned
            covered[start:start + count] += 1
            at += count
        assert at == off + n
    assert nxt == len(crows)
    want = torch.zeros_like(covered)
    for off, n in zip(offs, sizes):
        want[off:off + n] = 1
    assert torch.equal(covered, want)
    assert ops.grad_report_chunks([]) == ([], [])
    # the last chunk of C + 1 elements is the single element behind the boundary
    assert crows[prows[5][0] + 1] == (5, offs[5] + C, 1)
    for bad in ([(-8, 4)], [(0, -1)], [(0, 2 ** 31)]):
        with pytest.raises(ValueError):
            ops.grad_report_chunks(bad)


def test_no_cpu_path():
    from clover_amd import ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.grad_report_table([(0, 8)], 'cpu')
    tab = ops.GradReportTable(torch.tensor([0, 1, 0, 0, 8]), 1, 1, 8, (8,), 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.grad_report(torch.zeros(8), tab, torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=torch.int32), 1)


# ---------------------------------------------------------------------------------------------- 2. the hook
class FakeEngine:
    """An engine whose steps are skipped or taken as ``plan`` says (True: skipped)."""

    def __init__(self, plan, scale=1024.0):
        self.plan, self.scale = list(plan), scale
        self.calls = self.skipped = self.t = self.skip = 0
        self.reads = self.reports = 0

    def step(self, batch):
        self.skip = int(self.plan[self.calls])
        self.calls += 1
        self.skipped += self.skip
        self.t += 1 - self.skip
        return dict(loss=torch.zeros(()), log_vars=dict(loss=0.0), num_samples=1)

    def step_stats(self):
        self.reads += 1
        return dict(loss_scale=self.scale, grad_norm=float('inf') if self.skip else 2.5, skipped=self.skipped, t=self.t,
                    skip=self.skip, calls=self.calls)

    def overflow_report(self):
        self.reports += 1
        rows = [('a.weight', 10, 1, 3.0, 4.0), ('b.bias', 4, 3, 1.0, 1.0), ('c.weight', 6, 1, 5.0, 6.0),
                ('d.weight', 6, 2, 0.5, 0.6)]
        return dict(t=self.t, skipped=self.skipped, loss_scale=self.scale, rows=rows)


def run(plan, **kw):
    eng, out = FakeEngine(plan), []
    runner = CloverRunner(eng, model=torch.nn.Linear(2, 2), max_epochs=1)
    hook = OverflowHook(printer=out.append, **kw)
    log = LogHook(interval=1)
    runner.register_hook(log)
    runner.register_hook(hook)
    err = None
    try:
        runner.run([list(range(len(plan)))], [('train', 1)], 1)
    except RuntimeError as e:
        err = e
    return eng, hook, out, err, log


def test_hook_records_and_prints_only_when_skipped_grew():
    plan = [False, False, True, False, False, True, True, False]
    eng, hook, out, err, log = run(plan, interval=1, top=2)
    assert err is None
    assert len(hook.records) == len(plan) and eng.reads == len(plan) + 1        # ONE read per look (+ the baseline)
    for i, rec in enumerate(hook.records):
        assert set(rec) == {'epoch', 'iter', 'loss_scale', 'grad_norm', 'skipped'}
        assert rec['iter'] == i + 1 and rec['epoch'] == 1 and rec['loss_scale'] == 1024.0
        assert rec['skipped'] == sum(plan[:i + 1])
    assert len(out) == eng.reports == sum(plan)                                  # printed exactly on the skipped steps
    # the top rows: by non-finite count, then by magnitude
    lines = out[0].split('\n')
    assert len(lines) == 3 and lines[1].strip().startswith('b.bias') and lines[2].strip().startswith('d.weight')
    assert '1024' in lines[0]
    assert OverflowHook.top_rows(eng.overflow_report(), 4)[2:] == [('c.weight', 6, 1, 5.0, 6.0), ('a.weight', 10, 1, 3.0, 4.0)]
    # LogHook's records are what they were without the hook
    assert all(set(r) == {'epoch', 'iter', 'loss'} for r in log.records)
    # with an interval the looks thin out, and a look that finds no new skip prints nothing
    eng, hook, out, err, _ = run(plan, interval=4)
    assert len(hook.records) == 2 and eng.reads == 3 and len(out) == 2
    eng, hook, out, err, _ = run([False] * 6, interval=2)
    assert len(hook.records) == 3 and out == [] and eng.reports == 0


def test_consecutive_skip_error_fires_at_exactly_n():
    N = 3
    # N - 1 skips, a taken step, N - 1 skips: never N in a row
    eng, hook, out, err, _ = run([True, True, False, True, True, False, False], interval=1, max_consecutive_skips=N)
    assert err is None and eng.calls == 7 and hook.run_of_skips == 0
    # the N-th skip in a row stops the run right there
    eng, hook, out, err, _ = run([False, True, True, False, True, True, True, True, True], interval=1, max_consecutive_skips=N)
    assert isinstance(err, RuntimeError) and eng.calls == 7
    msg = str(err)
    assert '3 optimizer steps in a row' in msg and '1024' in msg and 'b.bias' in msg and 'max_consecutive_skips=3' in msg
    # without the limit the same plan runs through
    eng, hook, out, err, _ = run([True] * 9, interval=1)
    assert err is None and eng.calls == 9 and hook.run_of_skips == 9
    # windows of several steps: only all-skipped windows extend the run; a mixed one restarts it from the last step
    eng, hook, out, err, _ = run([True, True, True, False, True, True, True, True], interval=2, max_consecutive_skips=4)
    assert isinstance(err, RuntimeError) and eng.calls == 8
    eng, hook, out, err, _ = run([True, True, False, True, True, True], interval=2, max_consecutive_skips=4)
    assert err is None and hook.run_of_skips == 3


def test_hook_refuses_a_stepper_without_the_engine_interface():
    class Module(torch.nn.Linear):
        def train_step(self, batch, optimizer):
            return dict(loss=torch.zeros(()), log_vars={}, num_samples=1)
    m = Module(2, 2)
    runner = CloverRunner(m, model=m, max_epochs=1)
    runner.register_hook(OverflowHook(interval=1))
    with pytest.raises(TypeError, match='CloverEngine'):
        runner.run([[0]], [('train', 1)], 1)


# ---------------------------------------------------------------------------------------------- 3. tools/train.py
def _tool(name):
    spec = importlib.util.spec_from_file_location('clv_tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_registers_nothing_without_the_key():
    train = _tool('train')
    base = Config.fromfile(os.path.join(ROOT, 'configs', 'pretrain_synthetic.py'))
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'pretrain_overflow_report_synthetic.py'))
    assert base.get('overflow_report') is None
    assert train.overflow_hook(base) is None and train.engine_kwargs(base, 1e-4)['overflow_report'] is False
    hook = train.overflow_hook(cfg)
    assert isinstance(hook, OverflowHook) and train.engine_kwargs(cfg, 1e-4)['overflow_report'] is True
    want = dict(cfg.overflow_report)
    assert (hook.interval, hook.top, hook.max_consecutive_skips) == (want['interval'], want['top'],
                                                                     want['max_consecutive_skips'])
    assert hook.printer is print and train.overflow_hook(cfg, rank=1).printer is not print
    # the new config is the base one plus the key
    a, b = base.to_dict(), cfg.to_dict()
    assert {k: v for k, v in b.items() if k != 'overflow_report'} == a
    # the engine's switch is off by default
    import inspect
    from clover_amd.engine import CloverEngine
    assert inspect.signature(CloverEngine.__init__).parameters['overflow_report'].default is False


# ---------------------------------------------------------------------------------------------- 4. header and binding
CTYPES = {'const void*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64,
          'float': ctypes.c_float, 'double': ctypes.c_double, 'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p}


def test_header_prototype_matches_the_binding():
    from clover_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'clover_hip.h')).read()
    m = re.search(r'\bint\s+clv_grad_report\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'clv_grad_report is not declared'
    args = [a.strip().rsplit(' ', 1)[0].strip() for a in m.group(1).replace('\n', ' ').split(',')]
    res, argtypes = _lib.SIGNATURES['clv_grad_report']
    assert res is ctypes.c_int and [CTYPES[a] for a in args] == list(argtypes), args

    def const(name):
        return int(re.search(r'#define %s (\d+)' % name, hdr).group(1))
    assert const('CLV_GRAD_REPORT_HEADER_BYTES') == 4 * ops.GRAD_REPORT_HEADER_WORDS
    assert const('CLV_GRAD_REPORT_STAT_BYTES') == 4 * ops.GRAD_REPORT_STAT_WORDS
    assert const('CLV_GRAD_REPORT_PARAM_BYTES') == 16 and const('CLV_GRAD_REPORT_CHUNK_BYTES') == 24
    assert (const('CLV_GRAD_REPORT_F32'), const('CLV_GRAD_REPORT_HALF')) == (0, 1)
    assert const('CLV_OPTIM_STATE_BYTES') == ops.OPTIM_STATE_BYTES == 64
    for fname in ('libclover_hip_f16.so', 'libclover_hip.so'):
        so = ctypes.CDLL(os.path.join(ROOT, 'clover_amd', fname))
        fn = so.clv_grad_report
        fn.restype, fn.argtypes = res, argtypes
        # argument checks happen on the host, before any launch: null pointers and a mode outside {0, 1} are refused
        assert fn(None, 0, None, 0, 0, None, None, 0, None) == -1, fname
        assert fn(16, 0, 16, 1, 1, 16, 16, 2, None) == -1 and fn(16, 2, 16, 1, 1, 16, 16, 0, None) == -1, fname
        assert fn(16, 0, 12, 1, 1, 16, 16, 0, None) == -1 and fn(16, 0, 16, 0, 1, 16, 16, 0, None) == -1, fname
    # the dict of optim_state_read keeps its keys
    st = ops.optim_state_read(torch.zeros(16, dtype=torch.int32))
    assert set(st) == {'coef', 'bc1', 'bc2_sqrt', 'norm', 'skip', 't', 'skipped', 'loss_scale', 'scale_factor',
                       'scale_window', 'scale_iter', 'last_overflow', 'dynamic'}
