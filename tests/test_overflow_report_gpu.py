"""GPU tests of the overflow report: clv_grad_report (csrc/grad_report.hip) against torch on a buffer laid out like a gradient
slab, in fp32 and in the build's 16-bit element type, and the engine's use of it — which parameters a skipped step names,
eager and with captured graphs.  `-m gpu` only.

Bounds.  ``nonfinite`` and ``max_abs`` are exact (a count; a maximum, taken on bit patterns).  ``norm``: the kernel adds
non-negative fp32 squares in a fixed tree — per thread at most 16 vectors in sequence, then 6 + 2 tree levels, then the
chunks — so its sum of squares is within about (log2 n + 1) * 2^-24 < 2e-6 of the exact one; the tests ask for a relative
1e-5 against an fp64 sum, a factor of a few above that."""
import pytest
import torch

import closed_form as cf
import gutil

pytestmark = pytest.mark.gpu
DEV = 'cuda'
from clover_amd import _lib as _clv_lib  # noqa: E402
HALF = _clv_lib.half_dtype()          # the library's 16-bit element type

SIZES = (1, 7, 8, 255, 256, 16384, 16385, 40000)
SENTINEL = 0x5a5a5a5a
REL = 1e-5


def _layout():
    offs, pos = [], 0
    for n in SIZES:
        offs.append(pos)
        pos += (n + 7) // 8 * 8                            # 8-element aligned slots, as the slabs lay parameters out
    return offs, pos


_CASES = {}


def case(dtype):
    """(buffer on the host in `dtype`, reference) — built once per element type and never written again.  Finite values
    with denormals and -0.0 among them; NaN at element 0 of the 7-element parameter, +inf at the last element of the 16385
    one, -inf at elements 16383 and 16384 of the 40000 one (the two sides of a chunk boundary)."""
    if dtype in _CASES:
        return _CASES[dtype]
    offs, total = _layout()
    g = torch.Generator().manual_seed(20)
    x = (torch.randn(total, generator=g) * 3.0).to(dtype)
    denormal = torch.finfo(dtype).tiny / 4                 # below the smallest normal number of the type, representable
    for off, n in zip(offs, SIZES):
        if n >= 8:
            x[off + 1] = -0.0
            x[off + 2] = denormal
            x[off + n - 2] = -denormal
    x[offs[0]] = -0.0                                      # the 1-element parameter: nothing but a negative zero
    assert float(x[offs[2] + 2]) != 0.0 and abs(float(x[offs[2] + 2])) < torch.finfo(dtype).tiny
    x[offs[1]] = float('nan')
    x[offs[6] + 16384] = float('inf')
    x[offs[7] + 16383] = float('-inf')
    x[offs[7] + 16384] = float('-inf')
    ref = dict(nonfinite=[], max_abs=[], norm=[])
    for off, n in zip(offs, SIZES):
        v = x[off:off + n].float()
        fin = torch.isfinite(v)
        ref['nonfinite'].append(int((~fin).sum()))
        ref['max_abs'].append(v[fin].abs().max() if bool(fin.any()) else torch.zeros(()))
        ref['norm'].append(float(v[fin].double().pow(2).sum().sqrt()))
    assert ref['nonfinite'] == [0, 1, 0, 0, 0, 0, 1, 2]
    ref['max_abs'] = torch.stack(ref['max_abs'])
    _CASES[dtype] = (x, ref)
    return _CASES[dtype]


def make_state(skip, scale=512.0, t=3, skipped=2):
    from clover_amd import ops
    st = ops.optim_state_new(DEV)
    st[4], st[5], st[6] = int(skip), t, skipped
    st.view(torch.float32)[7] = scale                      # the scale the last prep's gradients carried
    st.view(torch.float32)[8] = scale                      # the current one
    return st


def device_buffer(dtype, shift=0):
    """The case's buffer on the device, `shift` elements behind a 16-byte boundary."""
    x, _ = case(dtype)
    room = torch.zeros(x.numel() + 8, dtype=dtype, device=DEV)
    assert room.data_ptr() % 16 == 0
    buf = room[shift:shift + x.numel()]
    buf.copy_(x)
    return buf


def check_report(rep, ref):
    assert rep['nonfinite'].tolist() == ref['nonfinite']
    # bit for bit: no rounding, no flushed denormal, no sign of a zero
    assert torch.equal(rep['max_abs'].view(torch.int32), ref['max_abs'].view(torch.int32)), (rep['max_abs'], ref['max_abs'])
    for i, (got, ss, want) in enumerate(zip(rep['norm'].tolist(), rep['sumsq'].tolist(), ref['norm'])):
        print(f'param {i} ({SIZES[i]} elements): norm {got!r}, fp64 {want!r}, rel {abs(got - want) / want if want else 0.0:.3g}')
        if want == 0.0:
            assert got == 0.0 and ss == 0.0
        else:
            assert abs(got - want) <= REL * want, (i, got, want)
            assert abs(ss ** 0.5 - want) <= REL * want, (i, ss, want)


@pytest.mark.parametrize('shift', [0, 1, 3])
@pytest.mark.parametrize('kind', ['f32', 'half'])
def test_kernel_report(kind, shift):
    """Mode 1 against torch; `shift` moves the buffer off the 16-byte boundary (the scalar head and tail of every chunk)."""
    from clover_amd import ops
    dtype = torch.float32 if kind == 'f32' else HALF
    _, ref = case(dtype)
    offs, _ = _layout()
    buf = device_buffer(dtype, shift)
    tab = ops.grad_report_table(list(zip(offs, SIZES)), DEV)
    assert tab.n_params == len(SIZES) and tab.n_chunks == 6 + 2 + 3
    out = ops.grad_report_new(tab, DEV)
    ops.grad_report(buf, tab, make_state(skip=0), out, 1)
    rep = ops.grad_report_read(out, tab)
    assert (rep['t'], rep['skipped'], rep['loss_scale'], rep['n_params']) == (3, 2, 512.0, len(SIZES))
    check_report(rep, ref)
    # the untouched parameters report no non-finite element; the lone negative zero reports 0 all over
    assert rep['nonfinite'][0] == 0 and float(rep['max_abs'][0]) == 0.0 and float(rep['norm'][0]) == 0.0
    # a pure function of the buffer: a second run into a fresh report gives the same bits, scratch records included
    out2 = ops.grad_report_new(tab, DEV)
    out2.fill_(SENTINEL)
    ops.grad_report(buf, tab, make_state(skip=0), out2, 1)
    assert torch.equal(out, out2)


@pytest.mark.parametrize('kind', ['f32', 'half'])
def test_mode_on_skip(kind):
    from clover_amd import ops
    dtype = torch.float32 if kind == 'f32' else HALF
    offs, _ = _layout()
    buf = device_buffer(dtype)
    tab = ops.grad_report_table(list(zip(offs, SIZES)), DEV)
    always = ops.grad_report_new(tab, DEV)
    ops.grad_report(buf, tab, make_state(skip=0), always, 1)
    out = ops.grad_report_new(tab, DEV)
    out.fill_(SENTINEL)
    ops.grad_report(buf, tab, make_state(skip=0), out, 0)          # a step that was taken: not a word is touched
    assert bool((out == SENTINEL).all())
    ops.grad_report(buf, tab, make_state(skip=1), out, 0)          # a skipped one: the whole report, as mode 1 writes it
    assert torch.equal(out, always)
    # the scale mode 0 reports is the one the gradients carried, not the one a dynamic scaler has moved to
    st = make_state(skip=1)
    st.view(torch.float32)[8] = 256.0
    ops.grad_report(buf, tab, st, out, 0)
    assert ops.grad_report_read(out, tab)['loss_scale'] == 512.0
    ops.grad_report(buf, tab, st, out, 1)
    assert ops.grad_report_read(out, tab)['loss_scale'] == 256.0


def test_empty_parameters_and_refusals():
    from clover_amd import ops
    buf = torch.ones(64, device=DEV)
    buf[40] = float('inf')
    tab = ops.grad_report_table([(0, 0), (8, 24), (32, 0), (32, 9)], DEV)
    assert (tab.n_params, tab.n_chunks, tab.extent) == (4, 2, 41)
    out = ops.grad_report_new(tab, DEV)
    ops.grad_report(buf, tab, make_state(skip=0), out, 1)
    rep = ops.grad_report_read(out, tab)
    assert rep['nonfinite'].tolist() == [0, 0, 0, 1]
    assert rep['max_abs'].tolist() == [0.0, 1.0, 0.0, 1.0] and rep['sumsq'].tolist() == [0.0, 24.0, 0.0, 8.0]
    with pytest.raises(ValueError, match='covers 41'):
        ops.grad_report(buf[:40], tab, make_state(skip=0), out, 1)
    with pytest.raises(ValueError, match='mode'):
        ops.grad_report(buf, tab, make_state(skip=0), out, 2)
    with pytest.raises(ValueError, match='out must be'):
        ops.grad_report(buf, tab, make_state(skip=0), out[:-1], 1)
    with pytest.raises(ValueError, match='buf must be'):
        ops.grad_report(buf.double(), tab, make_state(skip=0), out, 1)


def test_captured_report_follows_the_skip_flag():
    """Both passes inside one graph; `skip` is written 0, 1, 0 between three replays and the buffer changes every time: the
    report changes on the middle replay only, and then equals what an eager call gives."""
    from clover_amd import ops
    offs, _ = _layout()
    buf = device_buffer(torch.float32)
    tab = ops.grad_report_table(list(zip(offs, SIZES)), DEV)
    st = make_state(skip=0)
    out = ops.grad_report_new(tab, DEV)
    ops.grad_report(buf, tab, st, out, 0)                  # (loads the kernels ahead of the capture)
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        ops.grad_report(buf, tab, st, out, 0)
    assert bool((out == SENTINEL).all())                   # capturing runs nothing
    graph.replay()
    assert bool((out == SENTINEL).all())
    buf[offs[3] + 5] = float('nan')
    st[4] = 1
    graph.replay()
    want = ops.grad_report_new(tab, DEV)
    ops.grad_report(buf, tab, st, want, 1)
    assert torch.equal(out, want)
    assert ops.grad_report_read(out, tab)['nonfinite'].tolist() == [0, 1, 0, 1, 0, 0, 1, 2]
    buf[offs[4] + 5] = float('inf')
    st[4] = 0
    graph.replay()
    assert torch.equal(out, want)


# ---------------------------------------------------------------------------------------------- the engine
def make_model():
    import clover_amd
    m = clover_amd.build_model(cf.tiny_model_cfg())
    m.load_state_dict(cf.cf_state(gutil.manifest()), strict=False)
    return m.to(DEV).eval()          # eval: dropout off -> deterministic trajectories


def batch(B=2, tag='ovf'):
    return {k: v.to(DEV) for k, v in cf.cf_batch(B, tag=tag).items()}


def a_slot_the_norm_reads(eng):
    """(name, segment, offset, parameter) of a LayerNorm gain whose slab slot the norm pass reads: with the fused norm the
    first-touch weight gradients deliver their sums from the kernels that write them, so a value poked into one of THOSE
    slots afterwards is invisible to the skip decision — as it should be."""
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
def test_engine_names_the_parameter_behind_a_skipped_step(mode):
    from clover_amd.engine import CloverEngine
    b = batch()
    model = make_model()
    eng = CloverEngine(model, b, lr=1e-3, weight_decay=0.005, grad_clip=15.0, max_iters=10 ** 9, overflow_report=True)
    if mode == 'graph':
        eng.dry_step(b)
        assert eng.capture(b)
    assert eng.overflow_report() is None                   # nothing was skipped yet
    eng.step(b)
    assert eng.overflow_report() is None and eng.step_stats()['skipped'] == 0
    name, sg, off, p = a_slot_the_norm_reads(eng)
    # ---- an inf in ONE parameter's slot
    eng.forward_backward(b)
    at = off + p.numel() // 2
    sg.flat_g[at] = float('inf')
    slot = sg.flat_g[off:off + p.numel()].clone()
    weights = [s.flat_p.clone() for s in eng.segments]
    before = eng.step_stats()
    eng.optimizer_step()
    rep = eng.overflow_report()
    after = eng.step_stats()
    assert after['skipped'] == before['skipped'] + 1 == rep['skipped'] and after['t'] == before['t'] == rep['t']
    assert all(torch.equal(s.flat_p, w) for s, w in zip(eng.segments, weights))          # bit-unchanged
    assert rep['loss_scale'] == eng.loss_scale
    assert [r[0] for r in rep['rows']] == [name], rep['rows']
    _, numel, nonfinite, max_abs, norm = rep['rows'][0]
    assert (numel, nonfinite) == (p.numel(), 1)
    finite = slot[torch.isfinite(slot)].double()
    assert max_abs == pytest.approx(float(finite.abs().max()) / eng.loss_scale, rel=1e-6)
    assert norm == pytest.approx(float(finite.pow(2).sum().sqrt()) / eng.loss_scale, rel=REL)
    assert name in dict(model.named_parameters())
    # ---- a clean step leaves the report as it was
    eng.step(b)
    assert eng.step_stats()['t'] == after['t'] + 1 and eng.step_stats()['skipped'] == after['skipped']
    assert eng.overflow_report() == rep
    # ---- grad_stats(): every parameter, and the norm the optimizer then uses
    eng.forward_backward(b)
    stats = eng.grad_stats()
    eng.optimizer_step()
    gn = eng.grad_norm()
    assert [r[0] for r in stats['rows']] == [n for s in eng.segments for n in s.names]
    assert all(r[2] == 0 for r in stats['rows']) and stats['loss_scale'] == eng.loss_scale
    total = sum(r[4] ** 2 for r in stats['rows'])
    print(mode, 'sum of squared norms', total, 'grad_norm^2', gn * gn, 'rel', abs(total - gn * gn) / (gn * gn))
    assert abs(total - gn * gn) <= REL * gn * gn, (total, gn * gn)
    assert eng.overflow_report() == rep                    # grad_stats() writes a report of its own


def test_static_scale_that_overflows_reports_model_parameters():
    """A static loss scale far beyond fp16 (the 2**120 tests/test_engine_gpu.py starts its dynamic scaler from): every step
    is skipped, and what the report names are parameters of the model."""
    from clover_amd.engine import CloverEngine
    b = batch(tag='ovf-static')
    model = make_model()
    eng = CloverEngine(model, b, lr=1e-3, weight_decay=0.0, grad_clip=15.0, max_iters=10 ** 9, loss_scale=2.0 ** 120,
                       overflow_report=True)
    weights = [s.flat_p.clone() for s in eng.segments]
    eng.step(b)
    rep = eng.overflow_report()
    assert rep is not None and rep['skipped'] == 1 and rep['t'] == 0 and rep['loss_scale'] == 2.0 ** 120
    assert all(torch.equal(s.flat_p, w) for s, w in zip(eng.segments, weights))
    names = dict(model.named_parameters())
    assert all(r[0] in names and r[1] == names[r[0]].numel() and 1 <= r[2] <= r[1] for r in rep['rows'])
    if HALF == torch.float16:
        assert rep['rows']                                 # fp16 saturates long before 2**120
    eng.step(b)
    assert eng.overflow_report()['skipped'] == 2


def test_switch_off_launches_nothing_and_changes_nothing(monkeypatch):
    from clover_amd import ops
    from clover_amd.engine import CloverEngine
    b = batch(tag='ovf-off')
    on = CloverEngine(make_model(), b, lr=1e-3, weight_decay=0.0, grad_clip=15.0, max_iters=10 ** 9, overflow_report=True)
    out_on = on.step(b)
    real = ops.grad_report

    def refuse(*a, **k):
        raise AssertionError('clv_grad_report launched by an engine without overflow_report=True')
    monkeypatch.setattr(ops, 'grad_report', refuse)
    off = CloverEngine(make_model(), b, lr=1e-3, weight_decay=0.0, grad_clip=15.0, max_iters=10 ** 9)
    with pytest.raises(RuntimeError, match='overflow_report=True'):
        off.overflow_report()
    out_off = off.step(b)
    monkeypatch.setattr(ops, 'grad_report', real)
    # (the same forward on the same weights; approx only because a split reduction may add in another order)
    assert float(out_off['loss'].detach()) == pytest.approx(float(out_on['loss'].detach()), rel=1e-5)
    lv_on, lv_off = dict(out_on['log_vars']), dict(out_off['log_vars'])
    assert set(lv_on) == set(lv_off) and all(float(lv_off[k]) == pytest.approx(float(lv_on[k]), rel=1e-5, abs=1e-6)
                                             for k in lv_on)
    n_on, n_off = on.grad_norm(), off.grad_norm()
    assert abs(n_on - n_off) <= 1e-4 * n_off, (n_on, n_off)
    p_on, p_off = (torch.cat([s.flat_p for s in e.segments]) for e in (on, off))
    # Adam's first step is lr * sign(g): only gradients at rounding-noise level may differ between two runs
    assert float(((p_on - p_off).abs() > 1e-4).float().mean()) < 0.02
    assert off.step_stats()['t'] == 1 and off._report_out is None


def test_data_parallel_engine_reports_from_the_wire_copy(monkeypatch):
    """With a gradient exchange the norm, AdamW and therefore the report read the reduced 16-bit wire copy, not the fp32
    slabs: on a real 1-rank RCCL group, an inf written into the WIRE slot of one parameter skips the step and is named; one
    written into the fp32 slab behind the exchange is not seen, as the optimizer does not see it either."""
    import os
    import torch.distributed as dist
    from clover_amd.engine import CloverEngine
    b = batch(tag='ovf-dp')
    monkeypatch.setenv('CLOVER_FORCE_COLLECTIVES', '1')
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29567')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        model = make_model()
        eng = CloverEngine(model, b, lr=1e-3, weight_decay=0.0, grad_clip=15.0, max_iters=10 ** 9, bucket_mb=1,
                           overflow_report=True)
        assert eng.wire is not None and eng.reducer.active and eng.wire[0].dtype == HALF
        eng.step(b)
        assert eng.overflow_report() is None
        si, sg = 0, eng.segments[0]
        name, p, off = sg.names[1], sg.params[1], sg.offsets[1]
        # an inf in the fp32 slab AFTER the exchange: neither the optimizer nor the report reads it
        eng.forward_backward(b)
        torch.cuda.synchronize()
        sg.flat_g[off] = float('inf')
        eng.optimizer_step()
        assert eng.step_stats()['skipped'] == 0 and eng.overflow_report() is None
        # the same in the wire copy
        eng.forward_backward(b)
        torch.cuda.synchronize()
        eng.wire[si][off + p.numel() - 1] = float('inf')
        stats = eng.grad_stats()
        assert [(r[0], r[2]) for r in stats['rows'] if r[2]] == [(name, 1)]
        weights = [s.flat_p.clone() for s in eng.segments]
        eng.optimizer_step()
        rep = eng.overflow_report()
        assert eng.step_stats()['skipped'] == 1 and rep['skipped'] == 1
        assert [(r[0], r[1], r[2]) for r in rep['rows']] == [(name, p.numel(), 1)]
        assert all(torch.equal(s.flat_p, w) for s, w in zip(eng.segments, weights))
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
