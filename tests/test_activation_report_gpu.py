"""GPU tests of the activation report: clv_act_report / clv_act_report_latch (csrc/act_report.hip) against torch on the same
tensor, in fp32 and in the build's 16-bit element type, and the engine's use of them — which module a skipped step names as
the first with a non-finite output, eager and with captured graphs.  `-m gpu` only.

Bounds.  Every figure is exact: ``nonfinite`` is a count, ``max_abs`` a maximum taken on bit patterns, ``calls`` a count of
launches; the kernel accumulates no float and its atomics are integer add and integer max, which commute.  So every
comparison below is ``==`` on integers or on fp32 bit patterns."""
import os
import subprocess
import sys

import pytest
import torch

import closed_form as cf
import gutil

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from clover_amd import _lib as _clv_lib  # noqa: E402
HALF = _clv_lib.half_dtype()          # the library's 16-bit element type

SENTINEL = 0x5a5a5a5a
BLOCKS, THREADS, UNROLL = 256, 256, 2   # the launch shape of act_report.hip: grid bound, block, 16-byte loads per thread
BIG = 1_400_003                         # > BLOCKS * THREADS * UNROLL vectors of either type: the grid-stride loop comes
                                        # round again (fp32: twice unrolled + a rest, 16-bit: once + a rest), odd remainder


def kinds(kind):
    dtype = torch.float32 if kind == 'f32' else HALF
    return dtype, 128 // torch.finfo(dtype).bits      # elements per 16-byte vector


def counts(per):
    """0, 1, a vector -1 / 0 / +1, what one block takes in one pass -1 / 0 / +1, one vector more (a second block)."""
    w = THREADS * UNROLL * per
    return [0, 1, per - 1, per, per + 1, w - 1, w, w + 1, w + per, 3 * w + 5]


_BASE = {}


def base(dtype):
    """Finite random values on the host, built once per element type and never written again."""
    if dtype not in _BASE:
        g = torch.Generator().manual_seed(31)
        _BASE[dtype] = (torch.randn(BIG, generator=g) * 3.0).to(dtype)
    return _BASE[dtype]


def view(dtype, n, shift):
    """n elements of the base on the device, `shift` elements behind a 16-byte boundary."""
    room = torch.zeros(n + 16, dtype=dtype, device=DEV)
    assert room.data_ptr() % 16 == 0
    x = room[shift:shift + n]
    x.copy_(base(dtype)[:n])
    return x


def plant(x, shift, per, rotate=0):
    """The special values at the special places of the view: its first and last element, the unaligned head, the tail behind
    the last vector, both sides of the first block boundary.  Which value lands where rotates with `rotate`."""
    dtype, n = x.dtype, x.numel()
    fi = torch.finfo(dtype)
    values = [float('inf'), float('-inf'), float('nan'), -0.0, fi.tiny / 4, fi.max]
    head = min((per - shift) % per, n)
    nvec = (n - head) // per
    places = [0, n - 1, head - 1, head + nvec * per, head + THREADS * per - 1, head + THREADS * per]
    done = set()
    for j, at in enumerate(places):
        if 0 <= at < n and at not in done:
            done.add(at)
            x[at] = values[(j + rotate) % len(values)]
    return x


def expected(*xs):
    """[nonfinite, max_abs bits, calls, 0] of folding the tensors `xs` into a cleared record, from torch on the host."""
    v = torch.cat([x.detach().cpu().float().reshape(-1) for x in xs])
    fin = torch.isfinite(v)
    mx = v[fin].abs().max() if bool(fin.any()) else torch.zeros(())
    return [int((~fin).sum()), int(mx.reshape(1).view(torch.int32)), len(xs), 0]


def fold(*xs, slot=None):
    from clover_amd import ops
    if slot is None:
        slot = ops.act_report_new(1, DEV)[0]
    for x in xs:
        ops.act_report(x, slot[0])
    return slot


@pytest.mark.parametrize('kind', ['f32', 'half'])
def test_kernel_every_alignment_and_count(kind):
    """Every start 0 .. per - 1 elements behind a 16-byte boundary times every count that changes the launch: the record
    equals torch's, bit for bit, with the special values planted at the special places."""
    dtype, per = kinds(kind)
    for shift in range(per):
        for n in counts(per) + ([BIG] if shift in (0, 1, per - 1) else []):
            x = plant(view(dtype, n, shift), shift, per, rotate=shift)
            got = fold(x)[0].tolist()
            assert got == expected(x), (kind, shift, n, got, expected(x))


@pytest.mark.parametrize('kind', ['f32', 'half'])
def test_kernel_special_values(kind):
    dtype, per = kinds(kind)
    fi = torch.finfo(dtype)
    # nothing finite at all: max_abs stays 0
    x = torch.full((1000,), float('nan'), dtype=dtype, device=DEV)
    x[::3] = float('inf')
    x[1::3] = float('-inf')
    assert fold(x)[0].tolist() == [1000, 0, 1, 0]
    # zeros of both signs and one subnormal: the subnormal is the maximum, unflushed
    x = torch.zeros(777, dtype=dtype, device=DEV)
    x[5] = -0.0
    x[700] = -fi.tiny / 4
    want = expected(x)
    assert want[0] == 0 and 0 < want[1] and abs(float(x[700])) < fi.tiny
    assert fold(x)[0].tolist() == want
    x[700] = 0.0
    assert fold(x)[0].tolist() == [0, 0, 1, 0]              # a negative zero is a zero
    # the largest finite value of the type next to an infinity
    x[3], x[4] = -fi.max, float('inf')
    got = fold(x)[0]
    assert got.tolist() == expected(x) and float(got[1:2].view(torch.float32)) == fi.max and got[0] == 1


@pytest.mark.parametrize('kind', ['f32', 'half'])
def test_kernel_folds_and_repeats(kind):
    """Two launches on different tensors into one slot = the record of their concatenation with calls == 2; the same run
    into a cleared slot gives the same bits."""
    dtype, per = kinds(kind)
    a = plant(view(dtype, 70001, 3), 3, per, rotate=1)
    b = view(dtype, 4099, 0) * 2
    slot = fold(a, b)
    assert slot[0].tolist() == expected(a, b) and slot[0, 2] == 2
    again = fold(a, b)
    assert torch.equal(slot, again)
    slot.zero_()
    assert torch.equal(fold(a, b, slot=slot), again)
    # the neighbouring records of a table are left alone
    from clover_amd import ops
    live, _ = ops.act_report_new(3, DEV)
    live.fill_(SENTINEL)
    live[1].zero_()
    ops.act_report(a, live[1])
    assert live[1].tolist() == expected(a) and bool((live[0] == SENTINEL).all()) and bool((live[2] == SENTINEL).all())


def test_kernel_refusals():
    import ctypes as C
    from clover_amd import ops
    L = _clv_lib.lib()
    live, latched = ops.act_report_new(2, DEV)
    x = torch.ones(64, device=DEV)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)    # noqa: E731
    ok, arg, unsupported = 0, -1, -2
    assert L.clv_act_report(p(x), 64, 0, p(live), None) == ok
    assert L.clv_act_report(p(x), 64, 0, None, None) == arg                     # no slot
    assert L.clv_act_report(p(x), 64, 0, p(live, 4), None) == arg               # a slot off its 16-byte boundary
    assert L.clv_act_report(p(x), 64, 2, p(live), None) == arg                  # an unknown element type
    assert L.clv_act_report(p(x), -1, 0, p(live), None) == arg
    assert L.clv_act_report(None, 64, 0, p(live), None) == arg                  # no tensor, yet a count
    assert L.clv_act_report(p(x, 2), 8, 0, p(live), None) == arg                # fp32 off its 4-byte boundary
    assert L.clv_act_report(p(x, 1), 8, 1, p(live), None) == arg
    assert L.clv_act_report(p(x), 2 ** 31, 1, p(live), None) == unsupported     # the return code alone: nothing that large exists
    assert L.clv_act_report(None, 0, 0, p(live), None) == ok                    # count 0 is legal: it bumps calls
    torch.cuda.synchronize()
    assert live[0].tolist() == [0, 0x3f800000, 2, 0] and live[1].tolist() == [0, 0, 0, 0]
    st = ops.optim_state_new(DEV)
    assert L.clv_act_report_latch(None, p(live), p(latched), 2, None) == arg
    assert L.clv_act_report_latch(p(st), None, p(latched), 2, None) == arg
    assert L.clv_act_report_latch(p(st), p(live), None, 2, None) == arg
    assert L.clv_act_report_latch(p(st), p(live), p(latched, 4), 2, None) == arg
    assert L.clv_act_report_latch(p(st), p(live, 8), p(latched), 1, None) == arg
    assert L.clv_act_report_latch(p(st), p(live), p(latched), -1, None) == arg
    # the launchers refuse what the other ops refuse
    with pytest.raises(ValueError, match='contiguous fp32 or'):
        ops.act_report(x.double(), live[0])
    with pytest.raises(ValueError, match='contiguous fp32 or'):
        ops.act_report(torch.ones(8, 8, device=DEV)[:, ::2], live[0])
    with pytest.raises(ValueError, match='one record'):
        ops.act_report(x, live)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.act_report(x.cpu(), live[0])
    with pytest.raises(ValueError, match='latched must be'):
        ops.act_report_latch(st, live, latched[:-1], 2)


# ---------------------------------------------------------------------------------------------- the latch
def make_state(skip, scale=512.0, t=3, skipped=2):
    from clover_amd import ops
    st = ops.optim_state_new(DEV)
    st[4], st[5], st[6] = int(skip), t, skipped
    st.view(torch.float32)[7] = scale                      # the scale the last prep's gradients carried
    st.view(torch.float32)[8] = scale / 2                  # the current one: a dynamic scaler has moved already
    return st


def test_latch_on_skip_only():
    from clover_amd import ops
    live, latched = ops.act_report_new(3, DEV)
    a = plant(view(HALF, 5000, 1), 1, 8)
    ops.act_report(a, live[0])
    ops.act_report(view(torch.float32, 300, 0), live[2])
    latched.fill_(SENTINEL)
    ops.act_report_latch(make_state(skip=0), live, latched, 3)      # a step that was taken: not a byte is touched
    assert bool((latched == SENTINEL).all())
    ops.act_report_latch(make_state(skip=1), live, latched, 3)
    head = torch.tensor([3, 2, 0, 3, 0, 0, 0, 0], dtype=torch.int32)
    head.view(torch.float32)[2] = 512.0                             # the scale those gradients carried, not the moved one
    assert torch.equal(latched.cpu(), torch.cat([head, live.cpu().reshape(-1)]))
    rep = ops.act_report_read(latched, 3, latched=True)
    assert (rep['t'], rep['skipped'], rep['loss_scale'], rep['n_slots']) == (3, 2, 512.0, 3)
    assert rep['nonfinite'].tolist() == [expected(a)[0], 0, 0] and rep['calls'].tolist() == [1, 0, 1]
    now = ops.act_report_read(live, 3, latched=False)
    assert now['t'] is None and torch.equal(now['max_abs'], rep['max_abs']) and float(now['max_abs'][1]) == 0.0


def test_captured_report_follows_contents_and_skip_flag():
    """Clear + two scans + latch inside one graph; between the replays the tensors change and `skip` is written 0, 1, 0: the
    latched report changes on the middle replay only, and then holds what the tensors held at that replay."""
    from clover_amd import ops
    live, latched = ops.act_report_new(2, DEV)
    a, b = view(HALF, 9001, 2), view(torch.float32, 2049, 1)
    st = make_state(skip=0)

    def run():
        live.zero_()
        ops.act_report(a, live[0])
        ops.act_report(b, live[1])
        ops.act_report_latch(st, live, latched, 2)
    run()                                                  # (loads the kernels ahead of the capture)
    latched.fill_(SENTINEL)
    live.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        run()
    assert bool((latched == SENTINEL).all()) and bool((live == SENTINEL).all())         # capturing runs nothing
    graph.replay()
    assert bool((latched == SENTINEL).all())
    assert live.tolist() == [expected(a), expected(b)]
    a[4500] = float('nan')
    b[2048] = 1e30
    st[4] = 1
    graph.replay()
    want = [expected(a), expected(b)]
    assert want[0][0] == 1 and live.tolist() == want
    rep = ops.act_report_read(latched, 2, latched=True)
    assert rep['nonfinite'].tolist() == [1, 0] and float(rep['max_abs'][1]) == float(torch.tensor(1e30)) and rep['n_slots'] == 2
    kept = latched.clone()
    a[4501] = float('inf')
    st[4] = 0
    graph.replay()
    assert live.tolist() == [expected(a), expected(b)] and live[0, 0] == 2               # the live table follows ...
    assert torch.equal(latched, kept)                                                    # ... the latched report stays


@pytest.mark.skipif(os.environ.get('CLOVER_HALF', 'f16').lower() == 'bf16', reason='this process already runs the bf16 build')
def test_kernel_in_the_bf16_build():
    """One kernel case in a child process with CLOVER_HALF=bf16, started as tests/test_seq_parts_gpu.py starts its child."""
    env = dict(os.environ, CLOVER_HALF='bf16')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu', 'tests/test_activation_report_gpu.py', '-k',
                        'test_kernel_special_values and half'], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert '1 passed' in r.stdout, r.stdout[-2000:]


# ---------------------------------------------------------------------------------------------- the engine
LR = dict(lr=1e-3, weight_decay=0.005, grad_clip=15.0, max_iters=10 ** 9)
# (watched module X, a Linear bias inside it): a block of the last Swin stage, a text-encoder layer with a layer behind it,
# a fusion layer
PLANTS = {'swin': ('backbone.layers.1.blocks.0', 'mlp.fc2.bias'),
          'text': ('text_backbone.bert.encoder.layer.0', 'output.dense.bias'),
          'fusion': ('multimodal_backbone.bert_encoder.layer.0', 'output.dense.bias')}
TOWERS = ('backbone.', 'text_backbone.', 'multimodal_backbone.')
FORWARD_ORDER = {'backbone.': ['patch_embed', 'layers.0.blocks.0', 'layers.0.blocks.1', 'layers.0.downsample',
                               'layers.1.blocks.0', 'layers.1.blocks.1', 'norm'],
                 'text_backbone.': ['bert.embeddings', 'bert.encoder.layer.0', 'bert.encoder.layer.1'],
                 'multimodal_backbone.': ['fc_in', 'norm', 'bert_encoder.layer.0', 'bert_encoder.layer.1']}


def make_model():
    import clover_amd
    m = clover_amd.build_model(cf.tiny_model_cfg())
    m.load_state_dict(cf.cf_state(gutil.manifest()), strict=False)
    return m.to(DEV).eval()          # eval: dropout off -> deterministic trajectories


def batch(B=2, tag='act'):
    return {k: v.to(DEV) for k, v in cf.cf_batch(B, tag=tag).items()}


def make_engine(mode, b, model=None, **kw):
    from clover_amd.engine import CloverEngine
    eng = CloverEngine(model if model is not None else make_model(), b, **dict(LR, **kw))
    if mode == 'graph':
        eng.dry_step(b)
        assert eng.capture(b)
    return eng


def slab_slot(eng, pname):
    for sg in eng.segments:
        if pname in sg.names:
            return sg, sg.offsets[sg.names.index(pname)]
    raise AssertionError(f'{pname} is in no slab')


def torch_hooks(eng, names, maxima):
    """Independent bookkeeping for the eager comparison: torch forward hooks on the same modules — and, where the step enters
    a module through one of engine.ACT_ENTRY_METHODS instead of __call__ (torch's hooks do not see those calls), a wrapper of
    that method — keeping max |x| over the finite elements of every floating tensor of the output, with torch."""
    from clover_amd.engine import ACT_ENTRY_METHODS
    mods = dict(eng.model.named_modules())
    undo = []

    def walk(o):
        if torch.is_tensor(o):
            return [o] if o.is_floating_point() else []
        if isinstance(o, dict):
            o = list(o.values())
        return [t for v in o for t in walk(v)] if isinstance(o, (tuple, list)) else []

    def note(name, output):
        for t in walk(output):
            v = t.detach().float()
            fin = torch.isfinite(v)
            if bool(fin.any()):
                maxima[name] = max(maxima.get(name, 0.0), float(v[fin].abs().max()))

    for name in names:
        mod = mods[name]
        undo.append(mod.register_forward_hook(lambda _m, _i, out, name=name: note(name, out)).remove)
        for meth in ACT_ENTRY_METHODS:
            inner = getattr(mod, meth, None)
            if inner is None:
                continue

            def entry(*a, _inner=inner, _name=name, **k):
                out = _inner(*a, **k)
                note(_name, out)
                return out
            object.__setattr__(mod, meth, entry)
            undo.append(lambda mod=mod, meth=meth, inner=inner: object.__setattr__(mod, meth, inner))
    return undo


@pytest.mark.parametrize('mode', ['eager', 'graph'])
def test_clean_step_lists_every_watched_module(mode):
    b = batch()
    eng = make_engine(mode, b, overflow_report=True, activation_report=True)
    maxima, undo = {}, []
    if mode == 'eager':
        undo = torch_hooks(eng, eng._act.names, maxima)
    eng.step(b)
    for u in undo:
        u()
    assert eng.overflow_report() is None and eng.step_stats()['skipped'] == 0
    stats = eng.activation_stats()
    assert stats['limit'] == float(torch.finfo(HALF).max)
    names = [r[0] for r in stats['rows']]
    modules = dict(eng.model.named_modules())
    assert names and len(set(names)) == len(names) and all(n in modules for n in names)
    # every block-level module the step enters is there, each tower in forward order
    from clover_amd.engine import default_watched_modules
    assert set(names) <= set(default_watched_modules(eng.model))
    assert 'multimodal_backbone.bert_embedding' not in names          # never entered: the fusion encoder is fed embeddings
    assert {'mlm_head', 'ssl_head'} <= set(names)
    for tower, want in FORWARD_ORDER.items():
        assert [n for n in names if n.startswith(tower)] == [tower + w for w in want]
    for name, numel, calls, nonfinite, max_abs in stats['rows']:
        assert nonfinite == 0 and calls >= 1 and numel >= 1 and max_abs > 0.0, (name, numel, calls, max_abs)
    if mode == 'eager':
        for name, _, _, _, max_abs in stats['rows']:
            print(f'{name}: kernel max |x| {max_abs!r}, torch hooks {maxima.get(name)!r}')
            assert max_abs == maxima[name], (name, max_abs, maxima[name])        # floats of fp32 bit patterns: == is bit-equal
    # the table is cleared once per step: a second step on the same batch and (nearly) the same weights counts the same calls
    calls = {r[0]: r[2] for r in stats['rows']}
    eng.step(b)
    assert {r[0]: r[2] for r in eng.activation_stats()['rows']} == calls


@pytest.mark.parametrize('where', sorted(PLANTS))
@pytest.mark.parametrize('mode', ['eager', 'graph'])
def test_planted_nan_names_the_module(mode, where):
    from clover_amd.runner import OverflowHook
    X, bias = PLANTS[where]
    b = batch()
    eng = make_engine(mode, b, overflow_report=True, activation_report=True)
    eng.step(b)
    assert eng.overflow_report() is None
    order = [r[0] for r in eng.activation_stats()['rows']]
    sg, off = slab_slot(eng, f'{X}.{bias}')
    keep = (sg.flat_p[off].clone(), sg.shadow[off].clone())
    sg.flat_p[off] = float('nan')                          # the fp32 master and the 16-bit copy the kernels compute from
    sg.shadow[off] = float('nan')
    weights = [(s.flat_p.clone(), s.shadow.clone()) for s in eng.segments]
    before = eng.step_stats()
    eng.step(b)
    after = eng.step_stats()
    assert after['skipped'] == before['skipped'] + 1 and after['t'] == before['t']
    for s, (w, sh) in zip(eng.segments, weights):          # bit-unchanged, the plant included (NaN != NaN: compare the bits)
        assert torch.equal(s.flat_p.view(torch.int32), w.view(torch.int32))
        assert torch.equal(s.shadow.view(torch.int16), sh.view(torch.int16))
    rep = eng.overflow_report()
    act = rep['activations']
    assert act['first'] == X, act
    rows = act['rows']
    assert rows and all(r[3] > 0 and r[3] <= r[1] * r[2] for r in rows), rows
    named = [r[0] for r in rows]
    assert named == [n for n in order if n in named]       # forward order
    tower = next(t for t in TOWERS if X.startswith(t))
    upstream = [n for n in order[:order.index(X)] if n.startswith(tower)]
    assert upstream and not set(upstream) & set(named), (upstream, named)
    text = OverflowHook(printer=None).describe(rep)
    assert f'forward: first non-finite output at {X} ({rows[0][3]} of {rows[0][1] * rows[0][2]}), {len(rows) - 1} watched modules ' \
           'downstream' in text
    # ---- the value restored: a clean step leaves the report as it was
    sg.flat_p[off], sg.shadow[off] = keep
    eng.step(b)
    st = eng.step_stats()
    assert st['t'] == after['t'] + 1 and st['skipped'] == after['skipped']
    assert eng.overflow_report() == rep
    assert all(r[3] == 0 for r in eng.activation_stats()['rows'])


def a_slot_the_norm_reads(eng):
    """(name, segment, offset, parameter) of a slab slot the norm pass reads (as tests/test_overflow_report_gpu.py picks it):
    with the fused norm a value poked into a first-touch slot behind the backward is invisible to the skip decision."""
    fresh = getattr(eng, '_fresh_sinks', {}) if eng._norm_tables is not None else {}
    spans = [(si, off, off + n) for _, si, off, n in fresh.values()]
    found = None
    for si, sg in enumerate(eng.segments):
        for name, p, off in zip(sg.names, sg.params, sg.offsets):
            if any(sj == si and a <= off < b for sj, a, b in spans) or p.numel() < 2:
                continue
            if 'norm' in name and name.endswith('weight'):
                return name, sg, off, p
            found = found or (name, sg, off, p)
    assert found is not None
    return found


@pytest.mark.parametrize('mode', ['eager', 'graph'])
def test_gradient_side_overflow_reports_a_finite_forward(mode):
    from clover_amd.runner import OverflowHook
    b = batch()
    eng = make_engine(mode, b, overflow_report=True, activation_report=True)
    eng.step(b)
    name, sg, off, p = a_slot_the_norm_reads(eng)
    eng.forward_backward(b)
    sg.flat_g[off + p.numel() // 2] = float('inf')         # behind a clean backward, as the gradient report's test does
    eng.optimizer_step()
    rep = eng.overflow_report()
    assert rep is not None and [r[0] for r in rep['rows']] == [name]
    assert rep['activations'] == dict(first=None, rows=[])
    text = OverflowHook(printer=None).describe(rep)
    assert text.endswith('forward outputs all finite: the overflow arose in the backward pass or the loss')


def test_switch_off_launches_nothing(monkeypatch):
    from clover_amd import ops
    b = batch(tag='act-off')

    def refuse(*a, **k):
        raise AssertionError('the activation report launched in an engine without activation_report=True')
    monkeypatch.setattr(ops, 'act_report', refuse)
    monkeypatch.setattr(ops, 'act_report_latch', refuse)
    monkeypatch.setattr(ops, 'act_report_new', refuse)
    hooks_before = sum(len(m._forward_hooks) + len(m._forward_pre_hooks) for m in make_model().modules())
    eng = make_engine('eager', b, loss_scale=2.0 ** 120, overflow_report=True)
    assert eng._act is None
    assert sum(len(m._forward_hooks) + len(m._forward_pre_hooks) for m in eng.model.modules()) == hooks_before
    assert not any(meth in vars(m) for m in eng.model.modules() for meth in ('forward_pending', 'tokens', 'tokens_stacked'))
    eng.step(b)
    with pytest.raises(RuntimeError, match='activation_report=True'):
        eng.activation_stats()
    rep = eng.overflow_report()
    if HALF == torch.float16:                              # fp16 saturates long before 2**120: the step was skipped
        assert rep is not None
    assert rep is None or 'activations' not in rep
    plain = make_engine('eager', b)
    plain.step(b)
    assert plain.step_stats()['t'] == 1
    with pytest.raises(RuntimeError, match='overflow_report=True'):
        plain.overflow_report()
    with pytest.raises(ValueError, match='activation_report must be'):
        make_engine('eager', b, activation_report='yes')
    monkeypatch.undo()
    with pytest.raises(ValueError, match='matches no module'):
        make_engine('eager', b, activation_report=dict(modules=['no.such.module*']))


def test_extra_modules_by_pattern():
    b = batch()
    eng = make_engine('eager', b, activation_report=dict(modules=['text_backbone.bert.encoder.layer.*.attention']))
    eng.step(b)
    names = [r[0] for r in eng.activation_stats()['rows']]
    at = names.index('text_backbone.bert.encoder.layer.1.attention')          # inside its layer: it reports ahead of it
    assert names[at - 1:at + 2] == ['text_backbone.bert.encoder.layer.0', 'text_backbone.bert.encoder.layer.1.attention',
                                    'text_backbone.bert.encoder.layer.1']
    assert 'multimodal_backbone.bert_encoder.layer.0.attention' not in names and 'backbone.norm' in names
    # a module the step never calls cannot report: asking for it is refused, and the model is left without hooks
    model = make_model()
    with pytest.raises(ValueError, match='never calls a module matching'):
        make_engine('eager', b, model=model, activation_report=dict(modules=['*.pooler']))
    assert not any(m._forward_hooks or m._forward_pre_hooks for m in model.modules())
    assert not any(meth in vars(m) for m in model.modules() for meth in ('forward_pending', 'tokens', 'tokens_stacked'))
    # without overflow_report the table is live, nothing is latched, and overflow_report() says which keyword it needs
    with pytest.raises(RuntimeError, match='overflow_report=True'):
        eng.overflow_report()


@pytest.mark.parametrize('mode', ['eager', 'graph'])
def test_evaluation_leaves_the_table_alone(mode):
    b = batch()
    eng = make_engine(mode, b, overflow_report=True, activation_report=True)
    eng.step(b)
    torch.cuda.synchronize()
    live, latched = eng._act.live.clone(), eng._act.latched.clone()
    model = eng.model
    assert not model.training
    with torch.no_grad():
        model(b['imgs'], None, return_loss=False, token_ids=b['token_ids'], segment_ids=b['segment_ids'],
              input_mask=b['input_mask'])                                  # the test forward, as EvalHook's loop calls it
        model.train_step(b, None)                                          # and a training forward from outside the engine
    torch.cuda.synchronize()
    assert torch.equal(eng._act.live, live) and torch.equal(eng._act.latched, latched)


def test_virtual_ranks():
    k = 2
    bs = [batch(tag=f'act-vr{j}') for j in range(k)]
    one = make_engine('eager', bs[0], overflow_report=True, activation_report=True)
    one.step(bs[0])
    per_pass = {r[0]: r[2] for r in one.activation_stats()['rows']}
    eng = make_engine('eager', bs[0], virtual_ranks=k, overflow_report=True, activation_report=True)
    eng.step(bs)
    rows = eng.activation_stats()['rows']
    assert [r[0] for r in rows] == list(per_pass) and all(r[3] == 0 for r in rows)
    ratios = {r[2] / per_pass[r[0]] for r in rows}
    assert ratios == {float(2 * k - 1)}, ratios            # k forwards under no_grad / with the last alive, k - 1 recomputed
    X, bias = PLANTS['text']
    sg, off = slab_slot(eng, f'{X}.{bias}')
    sg.flat_p[off] = float('nan')
    sg.shadow[off] = float('nan')
    eng.step(bs)
    rep = eng.overflow_report()
    assert eng.step_stats()['skipped'] == 1 and rep['activations']['first'] == X
    assert all(r[2] == (2 * k - 1) * per_pass[r[0]] and r[3] > 0 for r in rep['activations']['rows'])
