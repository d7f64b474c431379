"""The activation report on the host: the two symbols in both libraries and in the binding, the unchanged ABI version,
OverflowHook's forward section on hand-made reports, the tools/train.py config key, and the default list of watched modules
(no GPU)."""
import ctypes
import importlib.util
import os
import re

import pytest

from clover_amd.runner import Config, OverflowHook

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {'const void*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64}


# ---------------------------------------------------------------------------------------------- 1. header, binding, libraries
def test_symbols_binding_and_abi_version():
    from clover_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'clover_hip.h')).read()
    assert _lib.ABI_VERSION == 20 and re.search(r'#define CLV_ABI_VERSION 20\b', hdr)
    sigs = {}
    for name in ('clv_act_report', 'clv_act_report_latch'):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, f'{name} is not declared'
        args = [a.strip().rsplit(' ', 1)[0].strip() for a in m.group(1).replace('\n', ' ').split(',')]
        res, argtypes = sigs[name] = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and [CTYPES[a] for a in args] == list(argtypes), (name, args)
    assert int(re.search(r'#define CLV_ACT_REPORT_SLOT_BYTES (\d+)', hdr).group(1)) == 4 * ops.ACT_REPORT_SLOT_WORDS == 16
    # the header names the reference lines the two entries stand in for
    doc = hdr[hdr.index('activation report (csrc/act_report.hip)'):hdr.index('int clv_act_report(')]
    assert 'fp16_utils.py:328-349' in doc and 'mmcv_Fp16OptimizerHook.py:123-141' in doc
    for fname in ('libclover_hip_f16.so', 'libclover_hip.so'):
        so = ctypes.CDLL(os.path.join(ROOT, 'clover_amd', fname))
        so.clv_abi_version.restype = ctypes.c_int
        assert so.clv_abi_version() == 20, fname
        scan, latch = so.clv_act_report, so.clv_act_report_latch          # AttributeError: the symbol is not exported
        scan.restype, scan.argtypes = sigs['clv_act_report']
        latch.restype, latch.argtypes = sigs['clv_act_report_latch']
        # argument checks happen on the host, before any launch
        assert scan(16, 8, 0, None, None) == -1 and scan(16, 8, 0, 24, None) == -1, fname       # no slot / a misaligned one
        assert scan(16, 8, 2, 32, None) == -1 and scan(16, -1, 0, 32, None) == -1, fname        # unknown elem / negative count
        assert scan(None, 8, 0, 32, None) == -1 and scan(18, 8, 0, 32, None) == -1, fname       # no tensor / a misaligned one
        assert scan(16, 2 ** 31, 1, 32, None) == -2, fname                                      # beyond INT32_MAX: unsupported
        assert latch(None, 16, 16, 1, None) == -1 and latch(16, None, 16, 1, None) == -1, fname
        assert latch(16, 16, None, 1, None) == -1 and latch(16, 16, 24, 1, None) == -1 and latch(16, 16, 16, -1, None) == -1


def test_no_cpu_path():
    import torch
    from clover_amd import ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.act_report_new(4, 'cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.act_report(torch.ones(8), torch.zeros(4, dtype=torch.int32))
    # the host reader needs no device: a latched buffer of two records, and the live table of the same
    buf = torch.zeros(8 + 8, dtype=torch.int32)
    buf[0], buf[1], buf[3] = 7, 2, 2
    buf.view(torch.float32)[2] = 1024.0
    buf[8:12] = torch.tensor([3, 0x42280000, 1, 0], dtype=torch.int32)          # 42.0
    rep = ops.act_report_read(buf, 2, latched=True)
    assert (rep['t'], rep['skipped'], rep['loss_scale'], rep['n_slots']) == (7, 2, 1024.0, 2)
    assert rep['nonfinite'].tolist() == [3, 0] and rep['max_abs'].tolist() == [42.0, 0.0] and rep['calls'].tolist() == [1, 0]
    live = ops.act_report_read(buf[8:].reshape(2, 4), 2, latched=False)
    assert live['t'] is None and live['max_abs'].tolist() == [42.0, 0.0]


# ---------------------------------------------------------------------------------------------- 2. the hook's text
REPORT = dict(t=11, skipped=3, loss_scale=1024.0,
              rows=[('backbone.layers.1.blocks.0.mlp.fc2.bias', 96, 96, 0.0, 0.0), ('mlm_head.decoder.weight', 4096, 17, 0.5, 2.0)])
TODAY = ('overflow: step skipped (3 so far, 11 taken) at loss_scale 1024; 2 parameter(s) with non-finite gradients, top 2:\n'
         '  backbone.layers.1.blocks.0.mlp.fc2.bias: 96 of 96 non-finite, max |g| 0, norm 0 over the finite ones\n'
         '  mlm_head.decoder.weight: 17 of 4096 non-finite, max |g| 0.5, norm 2 over the finite ones')


def test_describe_forward_section():
    hook = OverflowHook(printer=None)
    assert hook.describe(REPORT) == TODAY                 # without the key: today's text, to the letter
    rows = [('backbone.layers.1.blocks.0', 3072, 2, 64, 7.5), ('backbone.layers.1.blocks.1', 3072, 2, 6144, 0.0),
            ('backbone.norm', 1536, 1, 1536, 0.0)]
    first = dict(REPORT, activations=dict(first='backbone.layers.1.blocks.0', rows=rows))
    assert hook.describe(first) == TODAY + ('\nforward: first non-finite output at backbone.layers.1.blocks.0 (64 of 6144), '
                                            '2 watched modules downstream')
    clean = dict(REPORT, activations=dict(first=None, rows=[]))
    assert hook.describe(clean) == TODAY + '\nforward outputs all finite: the overflow arose in the backward pass or the loss'


class _Stepper:
    """What OverflowHook reads of a CloverEngine: every step is skipped, and the report names a first module (or not)."""
    def __init__(self, report):
        self.calls, self.report = 0, report

    def step_stats(self):
        return dict(loss_scale=1024.0, grad_norm=float('nan'), skipped=self.calls, t=0, skip=1, calls=self.calls)

    def overflow_report(self):
        return self.report


class _Runner:
    epoch, inner_iter = 0, 0

    def __init__(self, stepper):
        self.stepper = stepper


@pytest.mark.parametrize('with_first', [True, False])
def test_max_consecutive_skips_names_the_first_module(with_first):
    act = dict(first='text_backbone.bert.encoder.layer.0', rows=[('text_backbone.bert.encoder.layer.0', 512, 1, 9, 1.0)])
    report = dict(REPORT, activations=act) if with_first else dict(REPORT)
    said = []
    hook = OverflowHook(interval=1, max_consecutive_skips=2, printer=said.append)
    runner = _Runner(_Stepper(report))
    hook.before_run(runner)
    runner.stepper.calls = 1
    hook.after_train_iter(runner)
    runner.stepper.calls = 2
    with pytest.raises(RuntimeError) as err:
        hook.after_train_iter(runner)
    text = str(err.value)
    assert 'parameters with non-finite gradients: backbone.layers.1.blocks.0.mlp.fc2.bias, mlm_head.decoder.weight' in text
    if with_first:
        assert text.endswith('; first non-finite forward output: text_backbone.bert.encoder.layer.0')
        assert said[0].endswith('(9 of 512), 0 watched modules downstream')
    else:
        assert text.endswith('mlm_head.decoder.weight') and said[0] == TODAY


# ---------------------------------------------------------------------------------------------- 3. tools/train.py
def _tool(name):
    spec = importlib.util.spec_from_file_location('clv_tool_' + name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_parses_the_extended_key():
    train = _tool('train')
    base = Config.fromfile(os.path.join(ROOT, 'configs', 'pretrain_synthetic.py'))
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'pretrain_overflow_report_synthetic.py'))
    assert train.engine_kwargs(base, 1e-4)['activation_report'] is False
    assert train.engine_kwargs(cfg, 1e-4)['activation_report'] is False          # the committed config does not ask for it
    want = dict(cfg.overflow_report)
    cfg.overflow_report = dict(want, activations=True)
    kw = train.engine_kwargs(cfg, 1e-4)
    assert kw['activation_report'] is True and kw['overflow_report'] is True
    hook = train.overflow_hook(cfg)                        # the engine's keys do not reach the hook
    assert (hook.interval, hook.top, hook.max_consecutive_skips) == (want['interval'], want['top'],
                                                                     want['max_consecutive_skips'])
    cfg.overflow_report = dict(want, activations=True, modules=['backbone.layers.*.blocks.*.attn'])
    assert train.engine_kwargs(cfg, 1e-4)['activation_report'] == dict(modules=['backbone.layers.*.blocks.*.attn'])
    assert isinstance(train.overflow_hook(cfg), OverflowHook)
    cfg.overflow_report = dict(want, modules=['backbone.*'])
    with pytest.raises(ValueError, match='activations=True'):
        train.engine_kwargs(cfg, 1e-4)
    # the engine's switch is off by default
    import inspect
    from clover_amd.engine import CloverEngine
    assert inspect.signature(CloverEngine.__init__).parameters['activation_report'].default is False


# ---------------------------------------------------------------------------------------------- 4. what is watched
def test_default_watched_modules():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import closed_form as cf
    import clover_amd
    from clover_amd.engine import default_watched_modules
    model = clover_amd.build_model(cf.tiny_model_cfg())
    names = default_watched_modules(model)
    modules = dict(model.named_modules())
    assert len(set(names)) == len(names) and all(n in modules for n in names)
    assert {'backbone.patch_embed', 'backbone.layers.0.blocks.0', 'backbone.layers.0.blocks.1', 'backbone.layers.0.downsample',
            'backbone.layers.1.blocks.0', 'backbone.layers.1.blocks.1', 'backbone.norm', 'text_backbone.bert.embeddings',
            'text_backbone.bert.encoder.layer.0', 'text_backbone.bert.encoder.layer.1', 'multimodal_backbone.bert_embedding',
            'multimodal_backbone.bert_encoder.layer.0', 'multimodal_backbone.bert_encoder.layer.1', 'multimodal_backbone.fc_in',
            'multimodal_backbone.norm', 'mlm_head', 'ssl_head'} <= set(names)
    # heads only: the losses that are direct children too are not modules with an output to watch
    assert not {'loss_func', 'mlm_loss_func', 'ssl_loss'} & set(names)
