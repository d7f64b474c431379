"""The weight EMA on the GPU: the update and swap kernels against fp64 / bit patterns, the engine's average in eager and
hipGraph mode, checkpoints and `tools/train.py` with `ema_hook`, and the kernels once more in the bf16 build.  `-m gpu` only."""
import os
import subprocess
import sys

import pytest
import torch

from test_engine_gpu import batch, make_finetune_model, make_model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from clover_amd import _lib as _clv_lib  # noqa: E402
HALF = _clv_lib.half_dtype()
EPS = 2.0 ** -24                          # half an ulp of fp32, relative: one rounding
GUARD = 4                                 # untouched words before and after every entry


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Arena:
    """Entries laid out in one buffer with GUARD words of slack around each; ``off`` entries start 4 bytes (fp32) / 2 bytes
    (16-bit) behind a 16-byte boundary.  ``inside`` marks the words that belong to an entry."""

    def __init__(self, sizes, offs, dtype):
        self.spans, pos = [], 0
        for n, off in zip(sizes, offs):
            pos = (pos + GUARD + 7) // 8 * 8 + (1 if off else 0)           # 8 elements: 16 bytes of a 16-bit type too
            self.spans.append((pos, n))
            pos += n
        self.buf = torch.zeros(pos + GUARD + 8, device=DEV, dtype=dtype)
        assert self.buf.data_ptr() % 16 == 0
        self.inside = torch.zeros(self.buf.numel(), device=DEV, dtype=torch.bool)
        for a, n in self.spans:
            self.inside[a:a + n] = True

    def view(self, i):
        a, n = self.spans[i]
        return self.buf[a:a + n]

    def fill_random_bits(self, gen):
        bits(self.buf).copy_(torch.randint(-2 ** 31 if self.buf.dtype == torch.float32 else -2 ** 15,
                                           2 ** 31 if self.buf.dtype == torch.float32 else 2 ** 15, (self.buf.numel(),),
                                           generator=gen, device=DEV, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------- 4. update kernel
SLAB_SIZES = [8, 24, 4104, 2 ** 20 + 8]               # 16-byte aligned, multiples of 8, as the slabs are
LOOSE = [(1, False, False), (3, True, True), (49, False, False), (1000, True, False)]     # (n, p off, ema off)


def test_update_kernel_against_fp64():
    """20 updates of one table (slab-like entries: a chunk tail of 8, several chunks, 256 full chunks + 8; loose entries on
    the vector path with a tail and on the element path) with momenta of both schedules, p redrawn every time.  Per element
    |ema - fp64 recursion on the same fp32 inputs| <= 3 n 2^-24 max(|ema|, |p|) over the run after the n-th update: the kernel
    rounds (1 - m) -> fp32, (1 - m) ema, and the fused multiply-add (m -> fp32 adds m |p| 2^-24: (3 - m) roundings' worth at
    the most), and since 1 - m < 1 no earlier error grows.  Guard words around every entry stay bit-identical."""
    from clover_amd import ops
    from clover_amd.runner import ExpMomentumEMAHook, LinearMomentumEMAHook
    gen = torch.Generator(device=DEV).manual_seed(41)
    sizes = SLAB_SIZES + [n for n, _, _ in LOOSE]
    P = Arena(sizes, [False] * 4 + [po for _, po, _ in LOOSE], torch.float32)
    Em = Arena(sizes, [False] * 4 + [eo for _, _, eo in LOOSE], torch.float32)
    P.fill_random_bits(gen)
    Em.fill_random_bits(gen)
    idx = P.inside.nonzero().squeeze(1), Em.inside.nonzero().squeeze(1)

    def draw(A, where):                   # new values inside the entries; the guard words are not touched
        A.buf[where] = torch.randn(where.numel(), generator=gen, device=DEV)
    draw(P, idx[0])
    draw(Em, idx[1])
    entries = [(P.view(i), Em.view(i)) for i in range(len(sizes))]
    assert [P.view(i).data_ptr() % 16 for i in range(4, 8)] == [0, 4, 0, 4]
    assert [Em.view(i).data_ptr() % 16 for i in range(4, 8)] == [0, 4, 0, 0]
    table = ops.ema_table(entries, DEV)
    assert table.n_entries == 8 and table.n_blocks == 1 + 1 + 2 + 257 + 4 and table.numel == sum(sizes)
    p_guard, e_guard = bits(P.buf)[~P.inside].clone(), bits(Em.buf)[~Em.inside].clone()

    exp_a, exp_b = ExpMomentumEMAHook(), ExpMomentumEMAHook(momentum=0.01, total_iter=20)
    lin_a, lin_b = LinearMomentumEMAHook(), LinearMomentumEMAHook(momentum=0.5, warm_up=100)
    momenta = ([exp_a.momentum_fun(x) for x in range(7)] + [exp_b.momentum_fun(x) for x in range(6)]
               + [lin_a.momentum_fun(x) for x in range(3)] + [lin_b.momentum_fun(x) for x in range(4)])
    assert len(momenta) == 20 and momenta[0] > 0.999 and min(momenta) == 0.0002
    # entry space: the two arenas differ in length (their entries sit at different alignments), the elements INSIDE the
    # entries line up one to one in entry order
    ip, ie = idx
    ref = Em.buf[ie].double()
    big = torch.maximum(Em.buf[ie].abs(), P.buf[ip].abs()).double()
    worst = 0.0
    for n, m in enumerate(momenta, 1):
        draw(P, ip)
        ops.ema_update(table, m)
        pn = P.buf[ip].double()
        ref = (1.0 - m) * ref + m * pn
        big = torch.maximum(big, torch.maximum(ref.abs(), pn.abs()))
        err = (Em.buf[ie].double() - ref).abs()
        bound = 3 * n * EPS * big
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (n, m, float((err / bound).max()))
    print('update kernel: worst error / bound over 20 updates', worst)
    assert torch.equal(bits(P.buf)[~P.inside], p_guard) and torch.equal(bits(Em.buf)[~Em.inside], e_guard)
    # the average moved at all, everywhere
    assert float((Em.buf[ie] - P.buf[ip]).abs().max()) > 0


def test_update_kernel_refuses_bad_tables_and_momenta():
    from clover_amd import ops
    a, b = torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)
    with pytest.raises(ValueError):
        ops.ema_table([(a, b[:8])], DEV)
    with pytest.raises(ValueError):
        ops.ema_table([(a, a)], DEV)
    with pytest.raises(ValueError):
        ops.ema_table([(a, b.to(HALF))], DEV)
    with pytest.raises(ValueError):
        ops.ema_table([(a, b, torch.zeros(16, device=DEV))], DEV)              # an fp32 "shadow"
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.ema_table([(a.cpu(), b.cpu())], 'cpu')
    t = ops.ema_table([(a, b)], DEV)
    for m in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            ops.ema_update(t, m)
    empty = ops.ema_table([], DEV)
    ops.ema_update(empty, 0.5)
    ops.ema_swap(empty)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 5. swap kernel
# fp32 values whose 16-bit copy is decided by the rounding rule: signed zeros, infinities, the fp16 overflow boundary
# (65520 rounds to inf, 65519 does not), fp16 / bf16 / fp32 subnormals, ties, and the canonical quiet NaN
SPECIALS = [0.0, -0.0, float('inf'), -float('inf'), 65504.0, 65519.0, 65520.0, -65520.0, 1e-8, -1e-8, 5.96e-8, 2.98e-8,
            1e-40, -1e-40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -12, 3.0e38, 3.4e38,
            float('nan')]
# NaNs with payloads and signs (signalling ones too): exchanged bit for bit
NAN_BITS = [0x7F800001, 0x7FC12345, -1, -0x3ED000, 0x7FFFFFFF, -0x7FFFFF, 0x7FA00000]     # int32 views


def test_swap_kernel_bits_and_shadows():
    """p <-> ema bit for bit (random BIT patterns: NaN payloads, signalling NaNs, -0.0, subnormals), the 16-bit copy of the
    new p, two swaps = identity, entries without a shadow write nothing else.  What the 16-bit copy of a NaN WITH A PAYLOAD
    looks like is the one thing `p.to(HALF)` and the AdamW kernel's conversion do not share in the bf16 build (torch's bf16
    cast is software that returns the canonical 0x7FC0 for every NaN; the kernels' v_cvt_pk_bf16_f32 keeps sign and upper
    payload), so the shadowed entries carry every special value and the canonical NaN, and the payload NaNs sit in the
    entries without a shadow, where the exchange is what is checked."""
    from clover_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(43)
    # (n, p off, ema off, shadow: None / False aligned / True 2 bytes off)
    spec = [(8, False, False, False), (4104, False, False, False), (8200, False, False, False), (49, False, False, False),
            (77, True, False, False), (52, False, False, True),
            (1, False, False, None), (3, True, True, None), (49, False, False, None), (1000, True, False, None)]
    sizes = [s[0] for s in spec]
    P = Arena(sizes, [s[1] for s in spec], torch.float32)
    Em = Arena(sizes, [s[2] for s in spec], torch.float32)
    S = Arena(sizes, [bool(s[3]) for s in spec], HALF)
    for A in (P, Em, S):
        A.fill_random_bits(gen)
    shadowed = torch.zeros_like(S.inside)
    for i, s in enumerate(spec):
        if s[3] is None:                                    # NaNs with payloads among the random bits, plus these
            for A, rot in ((P, 0), (Em, 3)):
                v = bits(A.view(i))
                for j in range(min(v.numel(), len(NAN_BITS))):
                    v[j] = NAN_BITS[(j + rot) % len(NAN_BITS)]
            continue
        a, n = S.spans[i]
        shadowed[a:a + n] = True
        for A, rot in ((P, 0), (Em, 5)):                     # finite random values + the specials, no payload NaNs
            v = A.view(i)
            v.copy_(torch.randn(n, generator=gen, device=DEV) * 10.0 ** torch.randint(-6, 6, (n,), generator=gen, device=DEV))
            sp = torch.tensor(SPECIALS[rot:] + SPECIALS[:rot], device=DEV)[:n]
            v[:sp.numel()] = sp
        S.view(i).copy_(P.view(i).to(HALF))                  # the state the engine keeps: shadow = 16-bit copy of p
    assert bool(torch.isnan(P.buf[P.inside]).any()) and bool((bits(P.buf)[P.inside] == -2 ** 31).any())      # NaN, -0.0
    entries = [(P.view(i), Em.view(i), None if s[3] is None else S.view(i)) for i, s in enumerate(spec)]
    table = ops.ema_table(entries, DEV)
    assert table.shadow_numel == int(shadowed.sum())
    p0, e0, s0 = bits(P.buf).clone(), bits(Em.buf).clone(), bits(S.buf).clone()

    ops.ema_swap(table)
    assert torch.equal(bits(P.buf)[P.inside], e0[Em.inside]) and torch.equal(bits(Em.buf)[Em.inside], p0[P.inside])
    assert torch.equal(bits(P.buf)[~P.inside], p0[~P.inside]) and torch.equal(bits(Em.buf)[~Em.inside], e0[~Em.inside])
    for i, s in enumerate(spec):
        if s[3] is not None:
            assert torch.equal(bits(S.view(i)), bits(P.view(i).to(HALF))), (i, s)
    assert torch.equal(bits(S.buf)[~shadowed], s0[~shadowed])          # guards AND the slots of the entries without a shadow

    ops.ema_swap(table)
    assert torch.equal(bits(P.buf), p0) and torch.equal(bits(Em.buf), e0) and torch.equal(bits(S.buf), s0)


# ---------------------------------------------------------------------------------------------- 6. engine, eager
def floating_state(model, skip=()):
    return {n: t.detach().clone() for n, t in model.state_dict().items()
            if t.dtype.is_floating_point and n not in skip}


def test_engine_eager_average_follows_fp64_recursion():
    """Five optimizer steps with ema_update(0.5) after each (a large momentum makes a wrong formula visible); the third is
    made to overflow the way test_skipped_step_keeps_adam_count_and_dry_step_has_no_side_effects does it.  Every ema_*
    buffer equals the fp64 recursion over snapshots of this engine's own state_dict within test 4's bound."""
    from clover_amd.engine import CloverEngine
    b = batch(2, 'ema6')
    m = make_model()
    eng = CloverEngine(m, b, lr=1e-3, weight_decay=0.005, grad_clip=15.0, max_iters=10 ** 9)
    with pytest.raises(RuntimeError, match='ema_enable'):
        eng.ema_update(0.5)
    names0 = set(m.state_dict())
    eng.ema_enable()
    eng.ema_enable()                                                     # idempotent
    with pytest.raises(RuntimeError):
        eng.ema_enable(skip_buffers=True)
    state = floating_state(m, skip=set(eng.ema_names.values()))
    assert set(state) == set(eng.ema_names) == {n for n in names0 if m.state_dict()[n].dtype.is_floating_point}
    sd = m.state_dict()
    assert set(sd) == names0 | set(eng.ema_names.values())
    for n, en in eng.ema_names.items():
        assert en == 'ema_' + n.replace('.', '_') and torch.equal(sd[en], sd[n]) and sd[en].data_ptr() != sd[n].data_ptr()
    for sg in eng.segments:                                              # slab parameters: views into the ema slab
        for n, off in zip(sg.names, sg.offsets):
            assert sd[eng.ema_names[n]].data_ptr() == sg.ema.data_ptr() + 4 * off
    ref = {n: t.double() for n, t in state.items()}
    big = {n: t.abs().double() for n, t in state.items()}
    moved = 0.0
    for it in range(5):
        if it == 2:
            p0 = [sg.flat_p.clone() for sg in eng.segments]
            e0 = [sg.ema.clone() for sg in eng.segments]
            eng.model.train_step(b, None)['loss'].backward()
            (eng._zero_views[0] if eng._zero_views else eng.segments[0].flat_g)[7] = float('nan')
            eng.reducer.finish()
            eng.optimizer_step()
            assert all(torch.equal(sg.flat_p, q) for sg, q in zip(eng.segments, p0))       # the step was skipped ...
            assert eng.optimizer_state()['skipped'] == 1
        else:
            eng.step(b)
        eng.ema_update(0.5)
        if it == 2:                                                      # ... and the average still moved towards them
            for sg, q, e in zip(eng.segments, p0, e0):
                assert not torch.equal(sg.ema, e)
                assert float((sg.ema - q).abs().max()) < float((e - q).abs().max())
        now = floating_state(m, skip=set(eng.ema_names.values()))
        for n, t in now.items():
            ref[n] = 0.5 * ref[n] + 0.5 * t.double()
            big[n] = torch.maximum(big[n], torch.maximum(ref[n].abs(), t.abs().double()))
        moved = max(moved, max(float((now[n] - state[n]).abs().max()) for n in now))
    assert moved > 1e-3                                                  # the weights did train
    sd, worst = m.state_dict(), 0.0
    for n, en in eng.ema_names.items():
        err = (sd[en].double() - ref[n]).abs()
        bound = 3 * 5 * EPS * big[n]
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (n, float(err.max()), float(bound.max()))
    print('engine eager: worst error / bound', worst)
    assert eng.unused_names
    for n in eng.unused_names:                                           # never stepped: the average IS the parameter
        assert torch.equal(sd[eng.ema_names[n]], sd[n])


# ---------------------------------------------------------------------------------------------- 7. engine, graphs
def test_engine_swap_under_captured_graphs():
    from clover_amd.engine import CloverEngine
    b = batch(4, 'ema7')
    keys = ('imgs', 'token_ids', 'segment_ids', 'input_mask')
    m = make_finetune_model()
    eng = CloverEngine(m, b, lr=1e-3, weight_decay=0.005, grad_clip=15.0, max_iters=10 ** 9)
    eng.ema_enable()
    assert eng.capture(b)
    for _ in range(3):
        eng.step(b)
        eng.ema_update(0.5)
    captures = dict(eng._captures)
    fused = [f for sg in eng.segments for f in sg._fused]
    params = [p for sg in eng.segments for p in sg.params]
    with_t = [p for p in params + fused if hasattr(p, '_clv_shadow_t')]
    assert with_t and all(sg.shadow_t is not None for sg in eng.segments if sg._t_table is not None)
    before = [(sg.flat_p.clone(), sg.ema.clone(), sg.shadow.clone(), None if sg.shadow_t is None else sg.shadow_t.clone())
              for sg in eng.segments]
    with torch.no_grad():
        emb_raw = [t.clone() for t in m(return_loss=False, **{k: b[k] for k in keys})]

    eng.ema_swap()
    assert eng.ema_swapped
    for what in (lambda: eng.step(b), lambda: eng.forward_backward(b), eng.optimizer_step):
        with pytest.raises(RuntimeError, match='ema_swapped'):
            what()
    for sg, (p0, e0, s0, t0) in zip(eng.segments, before):
        assert torch.equal(bits(sg.flat_p), bits(e0)) and torch.equal(bits(sg.ema), bits(p0))
        assert torch.equal(bits(sg.shadow), bits(e0.to(HALF)))
    named = dict(m.named_parameters())
    sd = m.state_dict()
    for sg, (p0, e0, _, _) in zip(eng.segments, before):
        for n, off in zip(sg.names, sg.offsets):
            q = named[n]
            assert torch.equal(bits(q.data.reshape(-1)), bits(e0[off:off + q.numel()]))         # the pre-swap EMA
            assert torch.equal(bits(sd[eng.ema_names[n]].reshape(-1)), bits(p0[off:off + q.numel()]))
    for q in params + fused:
        assert torch.equal(bits(q._clv_shadow), bits(q.data.to(HALF)))
    for q in with_t:
        assert torch.equal(q._clv_shadow_t, q._clv_shadow.t().contiguous())
    with torch.no_grad():
        emb_ema = [t.clone() for t in m(return_loss=False, **{k: b[k] for k in keys})]
    assert all(bool(torch.isfinite(t).all()) for t in emb_ema)
    assert not any(torch.equal(a, r) for a, r in zip(emb_ema, emb_raw))

    eng.ema_swap()
    assert not eng.ema_swapped
    for sg, (p0, e0, s0, t0) in zip(eng.segments, before):
        assert torch.equal(bits(sg.flat_p), bits(p0)) and torch.equal(bits(sg.ema), bits(e0))
        assert torch.equal(bits(sg.shadow), bits(s0))
        assert t0 is None or torch.equal(bits(sg.shadow_t), bits(t0))
    losses = []
    for _ in range(2):
        losses.append(float(eng.step(b)['log_vars']['loss']))
        eng.ema_update(0.5)
    assert all(x == x and abs(x) < float('inf') for x in losses), losses
    assert set(eng._captures) == set(captures) and all(eng._captures[k] is captures[k] for k in captures)


# ---------------------------------------------------------------------------------------------- 8. checkpoints
def test_checkpoint_round_trip(tmp_path):
    from clover_amd.engine import CloverEngine
    from clover_amd.runner import CheckpointHook, CloverRunner, ExpMomentumEMAHook, Hook
    bs = [batch(2, f'ema8{i}') for i in range(2)]
    kw = dict(lr=1e-3, weight_decay=0.005, grad_clip=15.0, max_iters=10 ** 9)

    class Snapshot(Hook):
        """What the engine holds at the first before_train_epoch of epoch 2 (after the EMA hook's exchange)."""
        seen = None

        def before_train_epoch(self, runner):
            if runner.epoch == 1 and self.seen is None:
                eng = runner.stepper
                assert not eng.ema_swapped
                self.seen = [(sg.flat_p.clone(), sg.ema.clone(), sg.shadow.clone()) for sg in eng.segments]
                self.loose = {n: (t.clone(), runner.model.state_dict()[eng.ema_names[n]].clone())
                              for n, t in runner.model.state_dict().items() if n in eng.ema_names}

    def run(resume_from, work_dir):
        m = make_model()
        eng = CloverEngine(m, bs[0], **kw)
        runner = CloverRunner(eng, model=m, work_dir=str(work_dir), max_epochs=2)
        snap = Snapshot()
        runner.register_hook(CheckpointHook(str(work_dir)))
        runner.register_hook(snap)
        runner.register_hook(ExpMomentumEMAHook(momentum=0.01, total_iter=4, resume_from=resume_from), priority=49)
        runner.run([bs], [('train', 1)], 2)
        return eng, snap

    eng1, snap1 = run(None, tmp_path / 'a')
    ck = torch.load(str(tmp_path / 'a' / 'epoch_1.pth'), map_location='cpu')
    sd = ck['state_dict']
    floating = [n for n, t in sd.items() if t.dtype.is_floating_point and not n.startswith('ema_')]
    assert floating and set(eng1.ema_names) == set(floating)
    moved = 0.0
    for n in floating:
        en = 'ema_' + n.replace('.', '_')
        assert en in sd, n
        raw, ema = snap1.loose[n]                       # after the exchange back: parameters raw, ema_* the average
        assert torch.equal(sd[n], ema.cpu()), n         # the checkpoint's parameters are the average ...
        assert torch.equal(sd[en], raw.cpu()), n        # ... and its ema_* entries the raw weights
        moved = max(moved, float((raw - ema).abs().max()))
    assert moved > 0
    assert sorted(os.listdir(tmp_path / 'a')) == ['epoch_1.pth', 'epoch_2.pth']

    eng2, snap2 = run(str(tmp_path / 'a' / 'epoch_1.pth'), tmp_path / 'b')
    assert snap1.seen and snap2.seen and len(snap1.seen) == len(snap2.seen)
    for (p1, e1, s1), (p2, e2, s2) in zip(snap1.seen, snap2.seen):
        assert torch.equal(bits(p1), bits(p2)) and torch.equal(bits(e1), bits(e2)) and torch.equal(bits(s1), bits(s2))
    assert os.listdir(tmp_path / 'b') == ['epoch_2.pth']          # the resumed run went on with epoch 2 only


# ---------------------------------------------------------------------------------------------- 9. CLI
def test_tools_train_with_ema_hook(tmp_path):
    """tools/train.py on the EMA config, --validate, two short epochs: evaluation ran on the averaged weights (the printed
    metrics line carries the engine's ema_swapped), the best checkpoint holds ema_* entries; with ema_hook removed: neither."""
    cfg = os.path.join(ROOT, 'configs', 'finetune_retrieval_ema_synthetic.py')
    opts = ['videos_per_gpu=2', "log_config={'interval': 1}", "data.synthetic=[{'length': 2, 'frames': 8, 'tokens': 32}]",
            "data.synthetic_test={'pairs': 6, 'frames': 8, 'tokens': 32}"]

    def run(wd, extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), cfg, '--launcher', 'none', '--work_dir',
                            str(wd), '--validate', '--cfg-options', *opts, *extra], cwd=ROOT, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        recs = [eval(ln, {'nan': float('nan'), 'inf': float('inf')}) for ln in r.stdout.splitlines()
                if ln.startswith('{') and "'mode': 'val'" in ln]
        assert [rec['epoch'] for rec in recs] == [1, 2], r.stdout[-3000:]
        best = [f for f in os.listdir(wd) if '_best_' in f]
        assert len(best) == 1, os.listdir(wd)
        return recs, torch.load(os.path.join(str(wd), best[0]), map_location='cpu')['state_dict']

    recs, sd = run(tmp_path / 'ema', [])
    assert all(rec.get('ema') is True for rec in recs), recs
    floating = [n for n, t in sd.items() if t.dtype.is_floating_point and not n.startswith('ema_')]
    assert floating and all('ema_' + n.replace('.', '_') in sd for n in floating)
    assert any(not torch.equal(sd[n], sd['ema_' + n.replace('.', '_')]) for n in floating)

    recs, sd = run(tmp_path / 'plain', ['ema_hook=None'])
    assert all('ema' not in rec for rec in recs), recs
    assert not [n for n in sd if n.startswith('ema_')]


# ---------------------------------------------------------------------------------------------- 10. the bf16 build
@pytest.mark.skipif(os.environ.get('CLOVER_HALF', 'f16').lower() == 'bf16', reason='this process already runs the bf16 build')
def test_kernels_in_the_bf16_build():
    """The swap's 16-bit copy is the one part that depends on the element type: tests 4 and 5 once more in a child process
    on libclover_hip.so."""
    env = dict(os.environ, CLOVER_HALF='bf16')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu', 'tests/test_ema_gpu.py', '-k',
                        'test_update_kernel_against_fp64 or test_swap_kernel_bits_and_shadows'], env=env,
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert '2 passed' in r.stdout
