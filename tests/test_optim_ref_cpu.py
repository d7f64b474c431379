"""The references and input builders of tests/optim_ref.py, and the plan entry clv_optim_plan, without a GPU: the fp64
AdamW + prep model against torch.optim.AdamW with clip_grad_norm_, the scaler model against oracle/loss_scaler.py, the
conditions every builder promises, and that every size of the GPU suite reaches the launch class it is written for."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALVES = [torch.float16, torch.bfloat16]


def L():
    from clover_amd import _lib
    return _lib.lib()


def test_adamw64_and_prep_ref_equal_torch_adamw_over_four_steps_with_a_skip():
    b1, b2, eps, max_norm = R.f32(0.9), R.f32(0.98), R.f32(1e-8), R.f32(0.7)
    groups = [dict(n=37, lr=R.f32(1e-3), wd=R.f32(0.05)), dict(n=53, lr=R.f32(3e-4), wd=R.f32(0.0))]
    gen = torch.Generator().manual_seed(5)
    params = [torch.randn(g['n'], dtype=torch.float64, generator=gen).requires_grad_() for g in groups]
    opt = torch.optim.AdamW([dict(params=[p], lr=g['lr'], weight_decay=g['wd']) for p, g in zip(params, groups)],
                            betas=(b1, b2), eps=eps)
    mine = [dict(p=p.detach().numpy().copy(), m=np.zeros(g['n']), v=np.zeros(g['n'])) for p, g in zip(params, groups)]
    st = R.new_state()
    for step, scale in enumerate([3.0, 0.01, None, 1.0, 0.2]):            # clipped, not clipped, skipped, ...
        grads = [torch.randn(g['n'], dtype=torch.float64, generator=gen) * (scale or 1.0) for g in groups]
        raw = math.inf if scale is None else sum(R.sumsq64(g) for g in grads)
        st = R.prep_ref(st, raw, b1, b2, max_norm, 1.0)
        if scale is None:
            assert st['skip'] == 1
            continue                                                       # the reference does not call optimizer.step()
        for p, g in zip(params, grads):
            p.grad = g.clone()
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        assert st['skip'] == 0 and abs(st['norm'] - norm.item()) <= 1e-12 * norm.item()
        assert (st['coef'] < 1) == (norm.item() > max_norm)
        for me, g, grp, p in zip(mine, grads, groups, params):
            me['p'], me['m'], me['v'], _ = R.adamw64(me['p'], g, me['m'], me['v'], st['coef'], st['bc1'], st['bc2_sqrt'],
                                                     grp['lr'], b1, b2, eps, grp['wd'])
            s = opt.state[p]
            for got, want in ((me['p'], p.detach()), (me['m'], s['exp_avg']), (me['v'], s['exp_avg_sq'])):
                want = want.numpy()
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), step
    assert st['t'] == 4 and st['skipped'] == 1 and int(opt.state[params[0]]['step']) == 4


@pytest.mark.parametrize('init', [2.0 ** 20, 2.0])
def test_scaler_half_of_prep_ref_equals_the_oracle_loss_scaler(init):
    from oracle.loss_scaler import LossScaler
    ref = LossScaler(init_scale=init, mode='dynamic', scale_factor=2.0, scale_window=3)
    st = R.new_state(loss_scale=init, scale_factor=2.0, scale_window=3, last_overflow=-1, dynamic=1)
    floored = grew = False
    pattern = R.overflow_pattern()
    assert len(pattern) == 40
    for over in pattern:
        before = st['loss_scale']
        floored |= over and before / 2.0 < 1
        st = R.prep_ref(st, math.inf if over else 4.0, 0.9, 0.98, 1.0, 1.0)
        ref.update_scale(over)
        assert st['skip'] == int(over) and st['grad_loss_scale'] == before
        assert (st['loss_scale'], st['scale_iter'], st['last_overflow']) == (ref.cur_scale, ref.cur_iter, ref.last_overflow_iter)
        grew |= st['loss_scale'] > before
    assert grew and floored == (init == 2.0)                               # the floor at 1 is reached from 2
    assert st['t'] + st['skipped'] == 40 and st['skipped'] == sum(pattern)


def test_static_scaler_of_prep_ref_never_moves():
    from oracle.loss_scaler import LossScaler
    ref = LossScaler(init_scale=1024.0, mode='static')
    st = R.new_state(loss_scale=1024.0, scale_factor=2.0, scale_window=3, last_overflow=-1, dynamic=0)
    for over in R.overflow_pattern(8):
        st = R.prep_ref(st, math.inf if over else 1024.0 ** 2 * 9, 0.9, 0.98, 0.0, 1.0)
        ref.update_scale(over)
        assert (st['loss_scale'], st['scale_iter']) == (ref.cur_scale, ref.cur_iter) == (1024.0, 0)
        if not over:
            assert st['norm'] == 3.0 and st['coef'] == 1 / 1024.0          # divided out


def test_prep_ref_overflow_conditions():
    st = R.new_state()
    assert R.prep_ref(st, 3.2e38, 0.9, 0.98, 1.0, 2.0 ** -20)['skip'] == 1          # raw alone, the scaled sum is finite
    assert math.isfinite(R.prep_ref(st, 3.2e38, 0.9, 0.98, 1.0, 2.0 ** -20)['norm'])
    assert R.prep_ref(st, 1e30, 0.9, 0.98, 1.0, 1e5)['norm'] == math.inf            # the scaled sum overflows
    assert R.prep_ref(st, math.nan, 0.9, 0.98, 1.0, 1.0)['skip'] == 1
    assert R.prep_ref(st, 16.0, 0.9, 0.98, 0.0, 1 / 3)['coef'] == R.f32(1 / 3)      # max_norm = 0: coef is grad_scale


@pytest.mark.parametrize('n', sorted(R.SUMSQ_SIZES))
def test_integer_gradients_stay_under_the_cap(n):
    g = R.int_grad(n, n)
    assert g.dtype == np.float32 and (g == np.round(g)).all() and np.abs(g).max() <= 8
    assert 5 + R.sumsq64(g) < R.CAP
    for dt in HALVES:
        assert (torch.from_numpy(g).to(dt).float().numpy() == g).all()     # exact in either 16-bit type
    if n >= 1024:
        assert set(np.unique(g)) == {-8, -2, -1, 0, 1, 2, 8}


@pytest.mark.parametrize('bc2_sqrt', [math.sqrt(1 - 0.98), math.sqrt(1 - 0.98 ** 1000)])
def test_wide_state_reaches_every_regime(bc2_sqrt):
    p, g, m, v = R.wide_state(262147, 11, bc2_sqrt)
    for a in (p, g, m, v):
        nz = np.abs(a[a != 0])
        assert a.dtype == np.float32 and nz.min() >= np.finfo(np.float32).tiny           # normal or zero
    assert (v >= 0).all() and (p == 0).any() and (g == 0).any() and (v == 0).any()
    assert ((g == 0) & (m == 0) & (v == 0)).any() and ((g == 0) & (v == 0) & (m != 0)).any()
    assert ((g * m) > 0).any() and ((g * m) < 0).any()
    ag = np.abs(g[g != 0])
    assert ag.min() < 1e-8 and ag.max() > 10
    for coef in R.COEFS:
        _, m1, v1, sums = R.adamw64(p, g, m, v, coef, 0.1, bc2_sqrt, 1e-4, 0.9, 0.98, R.EPS, 0.05)
        r = np.sqrt(v1) / bc2_sqrt / R.EPS                                   # sqrt(v') / bc2_sqrt against eps
        assert (r < 1e-2).sum() > 100 and ((r > 0.5) & (r < 2)).sum() > 100 and (r > 1e4).sum() > 100
        # the products of adam_one stay normal as well
        gg = (1 - R.f32(0.98)) * (g.astype(np.float64) * coef) ** 2
        assert gg[gg > 0].min() > np.finfo(np.float32).tiny
        kappa = R.cancellation(sums[1], m1)
        assert 2.5 < kappa.max() <= R.KAPPA_MAX and R.p_cap(1.0) == R.R_P    # m' cancels, by a bounded factor


@pytest.mark.parametrize('dt', HALVES)
def test_pack_table_holds_every_value_and_every_tie(dt):
    x, K = R.pack_table(dt)
    assert K == (31744 if dt == torch.float16 else 32640) and x.dtype == torch.float32
    assert 2.5e5 < x.numel() < 2.7e5
    assert R.count_ties(x, dt) == 2 * K                                      # one midpoint above every finite magnitude
    y = x.to(dt)
    bits = y.view(torch.int16).to(torch.int32) & 0xffff
    every = set(bits.tolist())
    E, M, _ = R.half_layout(dt)
    inf = ((1 << E) - 1) << M
    assert all(k in every and (k | 0x8000) in every for k in range(K)) and inf in every and (inf | 0x8000) in every
    assert torch.isnan(y).sum() == 1 and torch.isinf(y).sum() > 4           # NaN, and overflow to +-inf
    # the reference conversion is round-to-nearest-even: every tie lands on an even pattern
    mid = x[1:8 * K:4]
    assert R.count_ties(mid, dt) == 2 * K and (mid.to(dt).view(torch.int16).to(torch.int32) & 1 == 0).all()
    lo, hi = x[2:8 * K:4], x[3:8 * K:4]
    hb = x[0:8 * K:4].to(dt).view(torch.int16).to(torch.int32) & 0xffff
    assert ((lo.to(dt).view(torch.int16).to(torch.int32) & 0xffff) == hb).all()            # just below the tie: down
    assert ((hi.to(dt).view(torch.int16).to(torch.int32) & 0xffff) == hb + 1).all()        # just above: up


def test_plan_symbol_in_header_binding_and_both_builds():
    from clover_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'clover_hip.h')).read()
    assert re.search(r'\bint clv_optim_plan\(int32_t kind, int64_t n, ClvOptimPlan\* out\);', hdr)
    assert 'clv_optim_plan' in _lib.SIGNATURES and C.sizeof(_lib.ClvOptimPlan) == 16
    for fname in ('libclover_hip.so', 'libclover_hip_f16.so'):
        so = C.CDLL(os.path.join(ROOT, 'clover_amd', fname))
        assert hasattr(so, 'clv_optim_plan'), fname


@pytest.mark.parametrize('kind, sizes', [(R.SUMSQ, R.SUMSQ_SIZES), (R.ADAMW, R.ADAMW_SIZES), (R.PACK, R.PACK_SIZES)])
def test_every_size_reaches_its_class_and_every_class_is_reached(kind, sizes):
    lib = L()
    for n, want in sizes.items():
        assert R.launch_class(R.plan(lib, kind, n), n) == want, (kind, n)
    reached = set(sizes.values())
    assert {R.TAIL_ONLY, R.ONE_BLOCK, R.MANY_BLOCKS} <= reached
    assert (R.TWO_TRIPS in reached) == (kind == R.SUMSQ)      # the other kernels start a second trip beyond 2^30 elements
    assert {n % 4 for n, c in sizes.items() if c != R.TAIL_ONLY} >= {0, 1, 3}


def test_plan_figures():
    lib = L()
    pl = R.plan(lib, R.SUMSQ, R.TWO_TRIP_N)
    assert (pl.grid, pl.block, pl.trips, pl.tail) == (2048, 256, 2, 3)
    assert R.TWO_TRIP_N == 4 * (2048 * 256 + 300) + 3 and R.TRIP2_FIRST == 4 * pl.grid * pl.block == 2097152
    assert R.sumsq_depth(pl) == 8 + 6 + 3 + 2048
    pl = R.plan(lib, R.SUMSQ, 262147)
    assert (pl.grid, pl.trips, pl.tail) == (256, 1, 3)
    pl = R.plan(lib, R.ADAMW, 262147)
    assert (pl.grid, pl.trips, pl.tail) == (256, 1, 3)
    pl = R.plan(lib, R.ADAMW, 2 ** 30)                        # the largest launch without a second trip
    assert (pl.grid, pl.trips) == (2 ** 20, 1)
    assert R.plan(lib, R.ADAMW, 2 ** 30 + 4).trips == 2
    assert R.plan(lib, R.PACK, 2 ** 30).grid == 2 ** 20
    assert R.plan(lib, R.PACK, 1027).grid == 2               # (n + 3) / 4 = 257 groups: the second workgroup is idle
    assert R.plan(lib, R.SUMSQ, 0).trips == 0


def test_plan_refusals():
    from clover_amd import _lib
    lib, out = L(), _lib.ClvOptimPlan()
    assert lib.clv_optim_plan(3, 4, C.byref(out)) == -1 and lib.clv_optim_plan(-1, 4, C.byref(out)) == -1
    assert lib.clv_optim_plan(0, -1, C.byref(out)) == -1 and lib.clv_optim_plan(0, 4, None) == -1
    # the pack kernel has no loop: beyond one 4-element group per thread of its largest grid it refuses, as clv_pack_bf16 does
    assert lib.clv_optim_plan(R.PACK, 2 ** 30 + 1, C.byref(out)) == -2
    one = C.c_void_p(16)                                                      # refused before anything is dereferenced
    assert lib.clv_pack_bf16(one, one, 2 ** 30 + 1, None) == -2
