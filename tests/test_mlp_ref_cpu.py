"""tests/mlp_ref.py without a GPU: the fp64 references against torch autograd (r = identity), the exact generators against
their caps at every shape tests/test_mlp_gpu.py uses, and every launch claim through the library's host entries
clv_rowgemm_plan / clv_mlp_fused_plan (a retuned launch fails HERE, on the claim, not quietly on another path)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import gemm_ref as gr
import mlp_ref as mr
import norm_ref as nr
from clover_amd import _lib

ERR_ARG, ERR_UNSUPPORTED = -1, -2
ALL_SMALL = [(K, mode, M) for (K, mode) in mr.SMALL for M in mr.SMALL_MS]


def L():
    return _lib.lib()


def rnd(seed, *shape, scale=1.0):
    return mr.gauss(seed, *shape, scale=scale).double()


def close(a, b, tol=1e-11):
    assert a.shape == b.shape
    assert (a - b).abs().max() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


# ----------------------------------------------------------------------------- the references against autograd
@pytest.mark.parametrize('with_res,with_k', [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize('gelu', [False, True])
def test_rowgemm_std_reference(gelu, with_res, with_k):
    M, N, K = 37, 24, 96
    a, res = rnd(1, M, K), (rnd(2, M, K) if with_res else None)
    k = torch.tensor([1.25, 0.0, 0.5] * 13)[:M] if with_k else None
    wt, bias = rnd(3, N, K, scale=0.1), rnd(4, N)
    o = mr.rowgemm_std(a, res, k, wt, bias, gelu, nr.ident)
    t = a * (k[:, None].double() if with_k else 1.0) + (res if with_res else 0.0)
    pre = F.linear(F.layer_norm(t, (K,), None, None, mr.EPS), wt, bias)
    close(o['y'], F.gelu(pre) if gelu else pre)
    close(o['s'], t)
    close(o['mean'], t.mean(-1))
    close(o['rstd'], (t.var(-1, unbiased=False) + mr.EPS).rsqrt())
    close(o['xhat'], F.layer_norm(t, (K,), None, None, mr.EPS))
    if gelu:
        close(o['pre'], pre)


def test_rowgemm_plain_reference():
    M, N, K = 19, 40, 128
    x, wt, bias = rnd(5, M, K), rnd(6, N, K, scale=0.1), rnd(7, N)
    pre = rnd(8, M, N).requires_grad_()
    acc = F.linear(x, wt, bias)
    close(mr.rowgemm_plain(x, wt, bias, None, nr.ident)['y'], acc)
    F.gelu(pre).backward(acc)                                   # d pre = upstream * gelu'(pre)
    close(mr.rowgemm_plain(x, wt, bias, pre.detach(), nr.ident)['y'], pre.grad)


@pytest.mark.parametrize('variant', mr.FM_VARIANTS)
@pytest.mark.parametrize('with_dsum', [False, True])
def test_one_kernel_references(variant, with_dsum):
    M, B = 48, 4
    a = rnd(11, M, mr.FM_C).requires_grad_()
    res = rnd(12, M, mr.FM_C).requires_grad_() if variant != 'plain' else None
    k = mr.factors(B).repeat_interleave(M // B) if variant == 'res_xscale' else None
    w1f, b1f = rnd(13, mr.FM_H, mr.FM_C, scale=0.12), rnd(14, mr.FM_H, scale=0.1)
    w2, b2 = rnd(15, mr.FM_C, mr.FM_H, scale=0.06), rnd(16, mr.FM_C, scale=0.1)
    dout, dsum = rnd(17, M, mr.FM_C), (rnd(18, M, mr.FM_C) if with_dsum else None)
    t = a * (k[:, None].double() if k is not None else 1.0) + (res if res is not None else 0.0)
    out = F.linear(F.gelu(F.linear(F.layer_norm(t, (mr.FM_C,), None, None, mr.EPS), w1f, b1f)), w2, b2)
    torch.autograd.backward([out, t], [dout, dsum if with_dsum else torch.zeros_like(t)])
    f = mr.mlp_fwd(a.detach(), None if res is None else res.detach(), k, w1f, b1f, w2, b2, nr.ident)
    close(f['out'], out.detach())
    close(f['s'], t.detach())
    b = mr.mlp_bwd(f['s'], f['mean'], f['rstd'], dout, dsum, k, w1f, b1f, w2, nr.ident)
    close(b['da'], a.grad, 1e-10)
    if res is not None:
        close(b['dres'], res.grad, 1e-10)
    close(b['act'], f['act'])
    close(b['xhat'], f['xhat'])
    if variant == 'res_xscale':
        assert b['da'][M // B:2 * (M // B)].abs().max() == 0           # the sample of factor 0
    # chunked evaluation is the same function
    c = mr.by_rows(lambda a_, r_, k_, *w: mr.mlp_fwd(a_, r_, k_, *w, nr.ident), [a.detach(), None if res is None else res.detach(), k],
                   [w1f, b1f, w2, b2], chunk=20)
    assert torch.equal(c['out'], f['out']) and torch.equal(c['mean'], f['mean'])


def test_the_floor_rounds_to_the_16_bit_grid():
    M, N, K = 33, 16, 96
    a, wt, bias = rnd(21, M, K).to(gr.HALF), rnd(22, N, K, scale=0.1).to(gr.HALF), rnd(23, N).float()
    e, f = (mr.rowgemm_std(a, None, None, wt, bias, True, r) for r in (nr.ident, gr.round16))
    for name in ('y', 'pre', 'xhat'):
        assert torch.equal(gr.round16(f[name]), f[name]) and not torch.equal(f[name], e[name])
        assert ((f[name] - e[name]).abs() <= 1.01 * nr.spacing16(e[name], gr.HALF) + 2e-3).all()
    assert torch.equal(f['mean'], e['mean']) and torch.equal(f['rstd'], e['rstd'])       # statistics of the unrounded t


# ----------------------------------------------------------------------------- the exact generators
def _check_std(c, gelu):
    M, K = c.t.shape
    assert set(c.t.unique().tolist()) <= {1.0, -1.0} and (c.t.sum(1) == 0).all()
    assert torch.unique(c.t, dim=0).shape[0] == M, 'two rows share a pattern'
    t = c.a.double() * (c.k.double()[:, None] if c.k is not None else 1.0) + (c.res.double() if c.res is not None else 0.0)
    assert torch.equal(t, c.t.double())
    if c.k is not None:
        dead = c.k == 0
        assert dead.any() and (~dead).any() and torch.equal(c.res[dead].double(), c.t[dead].double())
        assert c.a[dead].double().abs().max() > 2, 'the a operand of a dropped sample should be arbitrary'
    o = mr.rowgemm_std(c.a, c.res, c.k, c.wt, c.bias, gelu, gr.round16)
    assert torch.equal(o['xhat'], c.t.double()) and torch.equal(o['s'], c.t.double()) and (o['mean'] == 0).all()
    pre = c.acc + c.bias.double()
    assert torch.equal(o['pre'] if gelu else o['y'], pre), 'the pre-activation of the exact case is not a 16-bit value'
    gr.check_caps(c.t.to(gr.HALF), c.wt, c.bias, c.acc, c.q)
    if gelu:
        assert pre.abs().max() <= 16 and (M < 17 or pre.abs().max() >= 2)


@pytest.mark.parametrize('K,mode,M', ALL_SMALL)
def test_small_cases_meet_their_caps(K, mode, M):
    c = mr.small_case(K, mode, M)
    std, epi = mr.MODES[mode]
    if std:
        _check_std(mr.std_exact_case(c.M, c.N, c.K, epi == mr.EPI_GELU, c.res, c.samples), epi == mr.EPI_GELU)
    else:
        e = gr.exact_case(c.M, c.N, c.K, gelu=epi == mr.EPI_GELU_BWD)
        gr.check_caps(e.a, e.b, e.bias, e.acc, e.q)


@pytest.mark.parametrize('name', list(mr.TRIPS))
def test_trips_cases_meet_their_caps(name):
    c = mr.TRIPS[name]
    std, epi = mr.MODES[c.mode]
    if std:
        _check_std(mr.std_exact_case(c.M, c.N, c.K, epi == mr.EPI_GELU, c.res, c.samples), epi == mr.EPI_GELU)
    else:
        e = gr.exact_case(c.M, c.N, c.K, gelu=epi == mr.EPI_GELU_BWD)
        gr.check_caps(e.a, e.b, e.bias, e.acc, e.q)
        assert (e.acc + e.bias.double()).abs().max() / e.q <= gr.TOP


@pytest.mark.parametrize('M', list(mr.FM_CASES))
@pytest.mark.parametrize('variant', mr.FM_VARIANTS)
def test_one_kernel_exact_cases_meet_their_caps(M, variant):
    c = mr.fm_exact_case(M, variant)
    assert (c.t.sum(1) == 0).all() and torch.unique(c.t, dim=0).shape[0] == M
    t = c.a.double() * (c.k.double()[:, None] if c.k is not None else 1.0) + (c.res.double() if c.res is not None else 0.0)
    assert torch.equal(t, c.t.double())
    assert torch.equal(c.h * 16, (c.h * 16).round()) and c.h.abs().max() <= 16 and torch.equal(gr.round16(c.h), c.h)
    assert torch.equal(c.dact, c.dact.round()) and c.dact.abs().max() <= mr.FM_C
    fl = mr.mlp_bwd(c.t, torch.zeros(M), (torch.ones(M).double() + mr.EPS).rsqrt(), c.dout, None, c.k, c.w1f, c.b1f, c.w2, gr.round16)
    assert torch.equal(fl['xhat'], c.t.double()) and torch.equal(fl['h'], c.h) and torch.equal(fl['dact'], c.dact)
    if variant == 'res_xscale':
        assert ((c.k == 0).any() or M == 1) and mr.samples_of(M) * c.rps == M      # (M = 1: one sample, factor 1)


def test_caps_are_enforced_for_the_standardised_generator():
    ones = torch.ones(4, 512).to(gr.HALF)
    t = mr.pm1_rows(4, 512, torch.Generator().manual_seed(1)).to(gr.HALF)
    with pytest.raises(AssertionError, match='not every sum is a 16-bit value'):
        gr.check_caps(t, t, torch.zeros(4), gr.acc64(t, t), 1.0)            # a row against itself sums to 512
    with pytest.raises(AssertionError, match='not a multiple'):
        gr.check_caps(t, ones * 0.5, torch.zeros(4), gr.acc64(t, ones * 0.5) + 0.5, 1.0)


def test_sweep_points():
    p = mr.gelu_sweep_points()
    assert p.shape[1] == mr.FM_H and p.dtype == torch.float32 and p.numel() >= 12288 + 6 + 50 + 82
    flat = p.flatten().tolist()
    for v in (5.5, -5.5, 6.0, -6.0, 16.0, -16.0, 2.0 ** -24, -2.0 ** -24, 0.5):
        assert v in flat
    assert sum(1 for v in flat if 5.4999 < abs(v) < 5.5001) >= 6


# ----------------------------------------------------------------------------- the launch claims
@pytest.mark.parametrize('K,mode,M', ALL_SMALL)
def test_small_plans(K, mode, M):
    c = mr.assert_rg(mr.small_case(K, mode, M))
    assert c.claim.trips == 1 and c.N % 8 == 0 and c.N % c.claim.TN == 8 and c.claim.ny >= 2


@pytest.mark.parametrize('name', list(mr.TRIPS) + list(mr.STRIDED))
def test_trips_plans(name):
    c = mr.assert_rg(mr.TRIPS[name] if name in mr.TRIPS else mr.STRIDED[name])
    p = c.claim
    tiles = -(-c.M // 16)
    assert p.trips == -(-tiles // (p.gx * p.waves)) and p.ny == -(-c.N // p.TN)
    if name in mr.TRIPS:
        assert p.trips >= 2 and (c.M % 16 != 0 or c.N % p.TN != 0), 'a trips case needs a second tile per wave and a ragged last tile'


def test_plans_name_the_classes():
    """The facts the tables were built for, stated on the claims (which the tests above hold against the library)."""
    assert len(mr.SMALL) == 26
    assert {k for k, m in mr.SMALL if m in ('plain', 'dgelu')} == set(mr.KS_ALL)
    assert {k for k, m in mr.SMALL if m in ('std', 'std_gelu')} == set(mr.KS_STD)
    classes = {(m, v[1]) for (k, m), v in mr.SMALL.items()}
    assert classes == {(m, w) for m in mr.MODES for w in (4, 8, 12)}
    assert {(c.mode, c.claim.waves) for c in mr.TRIPS.values()} == classes, 'a (prologue, epilogue, waves) class has no trips case'
    # a trips case runs the instantiation the small table names for its (K, mode)
    for c in mr.TRIPS.values():
        TN, waves, ny, lds, gx = mr.SMALL[(c.K, c.mode)]
        assert (c.claim.TN, c.claim.waves, c.claim.lds) == (TN, waves, lds)
    # the XCD swizzle with whole groups of 8 row slices and a leftover, and with none
    assert any(c.claim.gx % 8 for c in mr.TRIPS.values()) and any(c.claim.gx % 8 == 0 for c in mr.TRIPS.values())
    x = mr.TRIPS['std_gelu-w8-k96']
    assert x.res and x.samples == 8 and (x.M // x.samples) % 16 != 0 and mr.FACTORS[1] == 0 and mr.FACTORS_EXACT[1] == 0
    assert set(mr.STRIDED) == set(mr.MODES)


@pytest.mark.parametrize('M', list(mr.FM_CASES))
def test_one_kernel_plans(M):
    p = mr.assert_fm(M)
    tiles = -(-M // 16)
    assert p.grid == min(tiles, 256) and p.tiles_min == tiles // p.grid and p.tiles_max == -(-tiles // p.grid)
    assert p.trips == -(-(-(-p.tiles_max // 2)) // 8)


def test_one_kernel_plans_name_the_bodies():
    c = mr.FM_CASES
    for M in (1, 16, 17):
        assert c[M].tiles_max == 1 and c[M].half_group == 1
    assert -(-4100 // 16) == 257 and (c[4100].tiles_min, c[4100].tiles_max) == (1, 2) and 4100 % 16 != 0
    assert c[8192].half_group == 0 and c[8192].tiles_min == 2
    assert c[12281].tiles_min == c[12281].tiles_max == 3
    assert -(-65550 // 16) == 4097 and c[65550].tiles_max == 17 and c[65550].trips == 2      # 9 groups: the ninth is half
    assert 69643 == 7 * 9949 and -(-69643 // 16) == 4353 and c[69643].tiles_max == 18 and c[69643].trips == 2
    assert all(c[M].trips == 1 for M in c if M <= 65536)
    # the sweep: M = 16 is the half-group body alone, M = 8192 the full-group body alone; M = 32 would NOT be
    assert mr.fm_plan(16) == mr.FmPlan(1, 1, 1, 1, 1) and mr.fm_plan(8192) == mr.FmPlan(256, 2, 2, 1, 0)
    assert mr.fm_plan(32) == mr.FmPlan(2, 1, 1, 1, 1)
    assert mr.GELU_SWEEP_MS == (16, 8192)


def test_plan_entries_refuse_what_the_kernels_refuse():
    p, q = _lib.ClvRowgemmPlan(), _lib.ClvMlpFusedPlan()
    assert C.sizeof(_lib.ClvRowgemmPlan) == 24 and C.sizeof(_lib.ClvMlpFusedPlan) == 20
    assert L().clv_rowgemm_plan(64, 64, 96, 0, 0, None) == ERR_ARG and L().clv_rowgemm_plan(0, 64, 96, 0, 0, p) == ERR_ARG
    for N, K, s in ((64, 160, 0), (64, 64, 0), (68, 96, 0), (0, 96, 0), (64, 288, 1), (64, 768, 1)):
        assert L().clv_rowgemm_plan(64, N, K, s, 0, p) == ERR_ARG and L().clv_rowgemm_supported(N, K, s) == 0
    for s, e in ((0, 1), (1, 2), (0, 3), (1, 3)):
        assert L().clv_rowgemm_plan(64, 64, 96, s, e, p) == ERR_UNSUPPORTED
    for K in mr.KS_ALL:
        for mode, (s, e) in mr.MODES.items():
            assert (L().clv_rowgemm_plan(64, 64, K, s, e, p) == 0) == ((K, mode) in mr.SMALL)
    assert L().clv_mlp_fused_plan(16, None) == ERR_ARG and L().clv_mlp_fused_plan(0, q) == ERR_ARG
    assert L().clv_mlp_fused_plan(-5, q) == ERR_ARG and L().clv_mlp_fused_plan(1, q) == 0


def test_a_retuned_launch_fails_the_claims(monkeypatch):
    real = L()

    class Retuned:
        def __getattr__(self, k):
            return getattr(real, k)

        def clv_rowgemm_plan(self, M, N, K, s, e, out):
            rc = real.clv_rowgemm_plan(M, N, K, s, e, out)
            out.waves = 4 if out.waves != 4 else 8
            return rc

        def clv_mlp_fused_plan(self, M, out):
            rc = real.clv_mlp_fused_plan(M, out)
            out.grid //= 2
            return rc

    monkeypatch.setattr(_lib, 'lib', lambda: Retuned())
    with pytest.raises(AssertionError, match='moved off the path'):
        mr.assert_rg(mr.TRIPS['plain-w8-k288'])
    with pytest.raises(AssertionError, match='claimed'):
        mr.assert_fm(8192)
