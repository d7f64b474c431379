"""The dual-softmax loss (csrc/losses.hip clv_dsl_loss_*) on every launch class of its two forms, through the C entries and
through clover_amd.ops.  Each case first asserts, through clv_dsl_loss_plan, the class it was written to reach, then
compares with the fp64 reference of tests/dsl_loss_ref.py.  The bounds are those of tests/LOSS_ERROR_BUDGET.md — 2 x the RMS
error of the fp32 floor, 4 x its per-row error, 4 x its loss error plus 2^-23 sqrt(2 G) — never a figure taken from the
kernels; tests/DSL_LOSS_ERROR_BUDGET.md has the reasoning and the measured table.

Kept property: both forms leave the same numbers in the same places of `work`, so the large backward accepts a work the small
forward filled and the other way round (test_backward_accepts_the_other_forms_work).  ops._kname names the attention
instantiations only; it does not apply to the loss kernels, whose classes are asserted through the plan record.  `-m gpu` only."""
import ctypes as C
import math

import pytest
import torch

import dsl_loss_ref as dr
import loss_ref as lr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL, TAIL = -7.0e30, 1024                  # floats beyond the work buffer, on the same allocation
RMS_X, ROW_X, LOSS_X = 2.0, 4.0, 4.0           # margins over the floor (LOSS_ERROR_BUDGET.md)


def L():
    from clover_amd import _lib
    return _lib.lib()


def T128():
    return int(L().clv_infonce_large_min_g())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Budget:
    """Collects (statistic, measured, allowed), prints the worst of each statistic, then asserts all of them."""

    def __init__(self, name):
        self.name, self.worst, self.bad = name, {}, []

    def check(self, stat, got, allowed, where=''):
        ratio = got / allowed if allowed > 0 else (0.0 if got == 0 else math.inf)
        if stat not in self.worst or ratio > self.worst[stat][0]:
            self.worst[stat] = (ratio, got, allowed)
        if not got <= allowed:
            self.bad.append((stat, where, got, allowed))

    def grad(self, stat, got, ref, floor, where=''):
        self.check(stat + '.rms', lr.rms_rel(got, ref), RMS_X * lr.rms_rel(floor, ref), where)
        self.check(stat + '.row', lr.row_stat(got, ref), ROW_X * lr.row_stat(floor, ref), where)

    def loss(self, stat, got, ref, floor, n, where=''):
        self.check(stat, lr.scalar_rel(got, ref), LOSS_X * lr.scalar_rel(floor, ref) + lr.ULP32 * math.sqrt(n), where)

    def done(self):
        print('DSLBUDGET', self.name, ' '.join(f'{k}={g:.3e}/{a:.3e}({r:.2f})' for k, (r, g, a) in sorted(self.worst.items())))
        assert not self.bad, self.bad[:8]


def work_buffer(G, Dm):
    """NaN where the kernels work, a sentinel in the TAIL floats behind it, one allocation."""
    floats = L().clv_dsl_loss_work_floats(G, Dm)
    w = torch.full((floats + TAIL,), float('nan'), device=DEV)
    w[floats:] = SENTINEL
    return w


def dsl_fwd(v, t, G, Dm, temperature, eps, T, large):
    lib = L()
    work = work_buffer(G, Dm)
    out = torch.full((1,), float('nan'), device=DEV)
    fn = lib.clv_dsl_loss_fwd_large if large else lib.clv_dsl_loss_fwd
    assert fn(ptr(v), ptr(t), ptr(out), ptr(work), G, Dm, temperature, eps, T, stream()) == 0
    return out, work


def dsl_bwd(work, G, Dm, temperature, T, large):
    lib = L()
    dout = torch.tensor([dr.DSL_DLOSS], device=DEV)
    dv, dt = torch.full((G, Dm), float('nan'), device=DEV), torch.full((G, Dm), float('nan'), device=DEV)
    fn = lib.clv_dsl_loss_bwd_large if large else lib.clv_dsl_loss_bwd
    assert fn(ptr(dout), ptr(work), ptr(dv), ptr(dt), G, Dm, temperature, T, stream()) == 0
    torch.cuda.synchronize()
    assert bool((work[-TAIL:] == SENTINEL).all())
    return dv, dt


def dsl_run(v, t, G, Dm, temperature, eps, T, large):
    """clv_dsl_loss_fwd / _bwd(_large).  -> (loss, dvideo, dtext)."""
    out, work = dsl_fwd(v, t, G, Dm, temperature, eps, T, large)
    dv, dt = dsl_bwd(work, G, Dm, temperature, T, large)
    return out.item(), dv, dt


def compare(bud, G, got, ref, floor, where):
    """got = (loss, dvideo, dtext) against the fp64 reference, bounded by the floor."""
    loss, dv, dt = got
    assert math.isfinite(loss), where
    bud.loss('loss', loss, ref['loss'].item(), floor['loss'].item(), 2 * G, where)
    rows = dr.dsl_clamp_rows(G)
    for name, g in (('dvideo', dv.cpu()), ('dtext', dt.cpu())):
        assert torch.isfinite(g).all(), (name, where)
        # the rows of norm 3e-10 / 3e-9 and the zero row have gradients orders above the others: each against itself
        keep = torch.ones(G, dtype=torch.bool)
        keep[rows[name]] = False
        bud.grad(name, g[keep], ref[name][keep], floor[name][keep], where)
        for row in rows[name]:
            bud.check(name + '.clamp', lr.row_stat(g[row][None], ref[name][row][None]),
                      ROW_X * lr.row_stat(floor[name][row][None], ref[name][row][None]), where + (row,))


def dsl_check(G, Dm, large, bud, hub=False):
    for temperature, eps in lr.NS_NORMS:
        for T in dr.DSL_TS:
            where = (temperature, eps, T, hub)
            v, t, ref, floor = dr.dsl_case_refs(G, Dm, temperature, eps, T, bool(large), hub)
            got = dsl_run(v.to(DEV), t.to(DEV), G, Dm, temperature, eps, T, large)
            compare(bud, G, got, ref, floor, where)


@pytest.mark.parametrize('G,Dm,path', [c[:3] for c in dr.DSL_CASES])
def test_dsl_loss(G, Dm, path):
    large = lr.path_is_large(path, G, T128())
    assert dr.dsl_claims()[(G, Dm, int(large))](dr.dsl_plan(L(), G, Dm, large))
    bud = Budget(f'dsl G{G} Dm{Dm} {"multi" if large else "one"}')
    dsl_check(G, Dm, large, bud)
    bud.done()


@pytest.mark.parametrize('G,Dm,path', [(33, 257, 'auto'), (65, 64, 'large')])
def test_dsl_loss_hub(G, Dm, path):
    """Video 0 is the mean of all text rows: a column of the cosine matrix without a dominant entry."""
    large = lr.path_is_large(path, G, T128())
    bud = Budget(f'dsl hub G{G} Dm{Dm} {"multi" if large else "one"}')
    dsl_check(G, Dm, large, bud, hub=True)
    bud.done()


def test_one_row_is_zero():
    """G = 1: every prior is 1, the loss and the gradients are zero."""
    for T in dr.DSL_TS:
        v, t = dr.dsl_inputs(1, 16)
        loss, dv, dt = dsl_run(v.to(DEV), t.to(DEV), 1, 16, 0.05, 1e-8, T, False)
        assert loss == 0.0 and not dv.any() and not dt.any()


def test_small_and_large_agree_at_the_threshold():
    """Both forms at G = 128, each within the bounds of its own floor against the same fp64 reference."""
    G, Dm = T128(), 64
    for large in (False, True):
        bud = Budget(f'dsl threshold G{G} {"multi" if large else "one"}')
        dsl_check(G, Dm, large, bud)
        bud.done()


@pytest.mark.parametrize('large', [False, True])
def test_bit_identical_over_two_runs(large):
    G, Dm, T = 131, 80, 20.0
    v, t = (x.to(DEV) for x in dr.dsl_inputs(G, Dm))
    a = dsl_run(v, t, G, Dm, 0.05, 1e-8, T, large)
    b = dsl_run(v, t, G, Dm, 0.05, 1e-8, T, large)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize('fwd_large', [False, True])
def test_backward_accepts_the_other_forms_work(fwd_large):
    G, Dm, temperature, eps, T = 65, 64, 0.05, 1e-8, 20.0
    v, t, ref, _ = dr.dsl_case_refs(G, Dm, temperature, eps, T, True)
    _, work = dsl_fwd(v.to(DEV), t.to(DEV), G, Dm, temperature, eps, T, fwd_large)
    dv, dt = dsl_bwd(work, G, Dm, temperature, T, not fwd_large)
    floor = dr.dsl_case_refs(G, Dm, temperature, eps, T, not fwd_large)[3]
    bud = Budget(f'dsl crossed fwd {"multi" if fwd_large else "one"}')
    rows = dr.dsl_clamp_rows(G)
    for name, g in (('dvideo', dv.cpu()), ('dtext', dt.cpu())):
        keep = torch.ones(G, dtype=torch.bool)
        keep[rows[name]] = False
        # the statistics come from the other form's forward: the floor of either order, whichever is larger
        other = dr.dsl_case_refs(G, Dm, temperature, eps, T, fwd_large)[3]
        bud.check(name + '.rms', lr.rms_rel(g[keep], ref[name][keep]),
                  RMS_X * max(lr.rms_rel(floor[name][keep], ref[name][keep]), lr.rms_rel(other[name][keep], ref[name][keep])))
    bud.done()


@pytest.mark.parametrize('G,Dm,force', [(33, 257, None), (128, 64, None), (65, 64, True), (256, 64, False)])
def test_through_ops(G, Dm, force):
    from clover_amd import ops
    large = force if force is not None else G >= T128()
    temperature, eps, T = 0.05, 1e-8, 20.0
    v, t, ref, floor = dr.dsl_case_refs(G, Dm, temperature, eps, T, bool(large))
    bud = Budget(f'dsl ops G{G} Dm{Dm} {"multi" if large else "one"}')
    old = ops.NCE_FORCE_LARGE
    ops.NCE_FORCE_LARGE = force
    try:
        vg, tg = v.to(DEV).requires_grad_(), t.to(DEV).requires_grad_()
        loss = ops.norm_softmax_loss(vg, tg, temperature=temperature, eps=eps, dual_softmax=T)
        (dr.DSL_DLOSS * loss).backward()
    finally:
        ops.NCE_FORCE_LARGE = old
    compare(bud, G, (loss.item(), vg.grad, tg.grad), ref, floor, (G, Dm, force))
    # the C entry of the same form, bit for bit
    direct = dsl_run(v.to(DEV), t.to(DEV), G, Dm, temperature, eps, T, large)
    assert direct[0] == loss.item() and torch.equal(direct[1], vg.grad) and torch.equal(direct[2], tg.grad)
    bud.done()


def test_ops_input_dtypes_follow_normsoftmax():
    """16-bit embeddings: computed in fp32, gradients returned in the inputs' dtypes."""
    from clover_amd import ops
    v, t = dr.dsl_inputs(8, 32)
    vg, tg = v.to(DEV).half().requires_grad_(), t.to(DEV).bfloat16().requires_grad_()
    loss = ops.norm_softmax_loss(vg, tg, temperature=0.05, eps=1e-8, dual_softmax=20.0)
    loss.backward()
    assert loss.dtype == torch.float32 and vg.grad.dtype == torch.float16 and tg.grad.dtype == torch.bfloat16
    want = dsl_run(vg.detach().float(), tg.detach().float(), 8, 32, 0.05, 1e-8, 20.0, False)
    assert loss.item() == want[0]


def test_without_dual_softmax_the_plain_entries_run_bit_for_bit():
    from clover_amd import ops
    lib = L()
    G, Dm, temperature, eps = 33, 257, 0.05, 1e-8
    v, t = (x.to(DEV) for x in lr.ns_inputs(G, Dm))
    vg, tg = v.clone().requires_grad_(), t.clone().requires_grad_()
    loss = ops.norm_softmax_loss(vg, tg, temperature=temperature, eps=eps, dual_softmax=None)
    (dr.DSL_DLOSS * loss).backward()
    work = torch.empty(lib.clv_normsoftmax_work_floats(G, Dm), device=DEV)
    out = torch.empty(1, device=DEV)
    assert lib.clv_normsoftmax_fwd(ptr(v), ptr(t), None, ptr(out), ptr(work), G, Dm, temperature, eps, stream()) == 0
    dout = torch.tensor([dr.DSL_DLOSS], device=DEV)
    dv, dt = torch.empty(G, Dm, device=DEV), torch.empty(G, Dm, device=DEV)
    assert lib.clv_normsoftmax_bwd(None, ptr(dout), ptr(work), ptr(dv), ptr(dt), None, G, Dm, temperature, stream()) == 0
    torch.cuda.synchronize()
    assert out.item() == loss.item() and torch.equal(dv, vg.grad) and torch.equal(dt, tg.grad)


def test_entries_refuse_bad_arguments():
    lib = L()
    G, Dm = 4, 16
    v, t = (x.to(DEV) for x in dr.dsl_inputs(G, Dm))
    work, out = work_buffer(G, Dm), torch.zeros(1, device=DEV)
    for T in (-1.0, float('inf'), float('nan')):
        for fn in (lib.clv_dsl_loss_fwd, lib.clv_dsl_loss_fwd_large):
            assert fn(ptr(v), ptr(t), ptr(out), ptr(work), G, Dm, 0.05, 1e-8, T, stream()) != 0
    assert lib.clv_dsl_loss_fwd(ptr(v), ptr(t), ptr(out), ptr(work), G, Dm, 0.0, 1e-8, 20.0, stream()) != 0
    assert lib.clv_dsl_loss_fwd(None, ptr(t), ptr(out), ptr(work), G, Dm, 0.05, 1e-8, 20.0, stream()) != 0
