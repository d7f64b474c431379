"""The references of tests/norm_ref.py themselves: ln_core against torch autograd, the gather against the oracle's, the
dropout mask's statistics, GELU against torch's.  Runs without a GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as nr
from oracle import indexing as ix


def rnd(*shape, scale=1.0, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def autograd_ln(x, res, k, gamma, beta, eps, dy, dy2, dsum, pre=None, post=None):
    """y = LN(pre(x k + res)); loss = <y, dy + dy2> + <x k + res, dsum> by autograd -> the dict ln_core returns."""
    xr = x.clone().requires_grad_()
    rr = res.clone().requires_grad_() if res is not None else None
    gr, br = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    t = xr * (k if k is not None else 1.0)
    if rr is not None:
        t = t + rr
    tg = pre(t) if pre else t
    y = F.layer_norm(tg, (tg.shape[-1],), gr, br, eps)
    loss = (y * (dy + (dy2 if dy2 is not None else 0.0))).sum()
    if dsum is not None:
        loss = loss + (t * dsum).sum()
    loss.backward()
    mu = tg.detach().mean(-1)
    var = tg.detach().var(-1, unbiased=False)
    return dict(y=y.detach(), s=t.detach(), mean=mu, rstd=(var + eps).rsqrt(), dgamma=gr.grad, dbeta=br.grad, dx=xr.grad,
                dres=rr.grad if rr is not None else None)


@pytest.mark.parametrize('rows,C', [(1, 2), (5, 8), (37, 100), (9, 264)])
@pytest.mark.parametrize('with_res,with_k,with_dy2,with_dsum',
                         [(0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 1, 0), (1, 1, 1, 1), (1, 1, 0, 0)])
def test_ln_core_equals_autograd(rows, C, with_res, with_k, with_dy2, with_dsum):
    x, dy = rnd(rows, C, seed=1), rnd(rows, C, seed=2)
    res = rnd(rows, C, seed=3) if with_res else None
    dy2 = rnd(rows, C, seed=4) if with_dy2 else None
    dsum = rnd(rows, C, seed=5) if with_dsum else None
    k = None
    if with_k:                          # a per-row scale (one row scaled by 0) times a dropout multiplier
        k = (torch.arange(rows, dtype=torch.float64) % 3 * 0.625)[:, None] * \
            (nr.ln_keep_mask(77, rows, C, 0.2).double() * nr.inv_keep(0.2))
    gamma, beta = 1 + 0.1 * rnd(C, seed=6), 0.1 * rnd(C, seed=7)
    # C = 2: xhat = +-1 up to eps, so d t is eps.rstd^2 times its terms — at eps = 1e-12 nothing but the cancellation residue
    # of either evaluation is left to compare
    for eps in (1e-5, 1e-12) if C > 2 else (1e-5,):
        want = autograd_ln(x, res, k, gamma, beta, eps, dy, dy2, dsum)
        for x_is_sum in (False, True):  # without rounding the stored sum IS the sum: the same function
            got = nr.ln_core(x, res, k, gamma, beta, eps, dy, dy2, dsum, nr.ident, x_is_sum)
            for name, w in want.items():
                if w is None:
                    # no residual operand: dres is d t itself; with k = 1 it equals dx
                    if k is None:
                        assert torch.equal(got['dres'], got['dx'])
                    continue
                assert rel(got[name], w) < 1e-10, (name, eps, x_is_sum, rel(got[name], w))


def test_rounding_hook_is_applied_where_the_kernels_store():
    """r = a 16-bit round trip: y, s, dx, dres are 16-bit values; the statistics are those of the UNROUNDED sum; and
    x_is_sum changes dgamma (the re-read sum) but not dbeta."""
    rows, C = 33, 48
    rt = lambda t: t.to(torch.bfloat16).double()      # noqa: E731
    x, res, dy = rt(rnd(rows, C, seed=1)), rt(rnd(rows, C, seed=2)), rt(rnd(rows, C, seed=3))
    gamma, beta = 1 + 0.1 * rnd(C, seed=6), 0.1 * rnd(C, seed=7)
    a = nr.ln_core(x, res, 1.25, gamma, beta, 1e-5, dy, None, None, rt, False)
    b = nr.ln_core(x, res, 1.25, gamma, beta, 1e-5, dy, None, None, rt, True)
    e = nr.ln_core(x, res, 1.25, gamma, beta, 1e-5, dy, None, None, nr.ident, False)
    for name in ('y', 's', 'dx', 'dres'):
        assert torch.equal(a[name], rt(a[name])), name
        assert 0 < rel(a[name], e[name]) < 2 ** -7, name
    assert torch.equal(a['mean'], e['mean']) and torch.equal(a['rstd'], e['rstd'])
    assert torch.equal(a['dgamma'], e['dgamma']) and torch.equal(b['dbeta'], e['dbeta'])
    assert 0 < rel(b['dgamma'], e['dgamma']) < 2 ** -7


@pytest.mark.parametrize('shape', [(1, 1, 2, 2, 8), (2, 3, 6, 10, 32)])
def test_gather_is_the_oracles_and_scatter_inverts_it(shape):
    x = rnd(*shape, seed=11)
    g = nr.merge_gather(x)
    want = ix.patch_merging_gather(x.numpy())
    assert np.array_equal(g.numpy(), want.reshape(-1, 4 * shape[-1]))
    assert torch.equal(nr.merge_scatter(g, shape), x)


@pytest.mark.parametrize('with_res,with_scale', [(0, 0), (1, 1)])
def test_gathered_ln_equals_autograd(with_res, with_scale):
    shape = (2, 1, 4, 6, 8)
    B, C4 = shape[0], 4 * shape[-1]
    x, res = rnd(*shape, seed=1), (rnd(*shape, seed=2) if with_res else None)
    k5 = torch.tensor([0.0, 1.25], dtype=torch.float64).view(B, 1, 1, 1, 1).expand(shape) if with_scale else None
    gamma, beta = 1 + 0.1 * rnd(C4, seed=6), 0.1 * rnd(C4, seed=7)
    dy = rnd(x.numel() // C4, C4, seed=3)
    want = autograd_ln(x, res, k5, gamma, beta, 1e-5, dy, None, None, pre=nr.merge_gather)
    got = nr.ln_core(nr.merge_gather(x), nr.merge_gather(res) if with_res else None,
                     nr.merge_gather(k5) if with_scale else None, gamma, beta, 1e-5, dy, None, None, nr.ident, False)
    assert rel(got['y'], want['y']) < 1e-10
    assert rel(got['dgamma'], want['dgamma']) < 1e-10 and rel(got['dbeta'], want['dbeta']) < 1e-10
    assert rel(nr.merge_scatter(got['dx'], shape), want['dx']) < 1e-10
    if with_res:
        assert rel(nr.merge_scatter(got['dres'], shape), want['dres']) < 1e-10
    if with_scale:
        assert (nr.merge_scatter(got['dx'], shape)[0] == 0).all()


@pytest.mark.parametrize('p', [0.1, 0.2, 0.5])
@pytest.mark.parametrize('seed', [0, 0x1234ABCD9E3779B9, 0xFFFFFFFFFFFFFFFF])
def test_keep_mask_statistics(p, seed):
    rows, C = 1000, 264
    m = nr.ln_keep_mask(seed, rows, C, p)
    n = rows * C
    assert abs(m.double().mean().item() - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n)
    assert torch.equal(m, nr.ln_keep_mask(seed, rows, C, p))              # a pure function of its arguments
    assert torch.equal(m[:17, :8], nr.ln_keep_mask(seed, 17, 8, p))       # ... of (row, column), not of the shape
    other = nr.ln_keep_mask(seed ^ (1 << 40), rows, C, p)                 # the high word of the seed takes part
    assert 0.2 * n * p * (1 - p) < (m != other).sum().item()


def test_keep_mask_against_a_scalar_restatement():
    """The tensor form against the kernel's formula written out with Python integers, element by element."""
    def one(seed, row, col, thresh):
        M = 0xFFFFFFFF
        x = ((row * 0x9E3779B1) & M) ^ ((col * 0x85EBCA77) & M) ^ (seed & M)
        x ^= x >> 16
        x = (x * 0x7feb352d) & M
        x ^= x >> 15
        x = (x * 0x846ca68b) & M
        x ^= x >> 16
        x = (x + (seed >> 32)) & M
        x ^= x >> 15
        x = (x * 0x2c1b3c6d) & M
        x ^= x >> 12
        return x >= thresh
    seed, p = 0xFEDCBA9876543210, 0.2
    thresh = int(float(np.float32(p)) * 4294967296.0)
    m = nr.ln_keep_mask(seed, 40000, 3, p)
    for row in (0, 1, 2, 777, 36864, 39999):
        for col in range(3):
            assert bool(m[row, col]) == one(seed, row, col, thresh), (row, col)
    m = nr.ln_keep_mask(seed, 3, 3072, p)
    for col in (0, 7, 8, 519, 3071):
        assert bool(m[2, col]) == one(seed, 2, col, thresh), col


def test_gelu_references():
    x = torch.linspace(-12, 12, 4801, dtype=torch.float64)
    assert rel(nr.gelu64(x), F.gelu(x)) < 1e-14
    xr = x.clone().requires_grad_()
    F.gelu(xr).sum().backward()
    assert rel(nr.gelu_grad64(x), xr.grad) < 1e-14
    # the negative tail, where 1 + erf cancels: x Phi(x) ~ -phi(x) (1 - 1/x^2 + 3/x^4) keeps its relative accuracy
    t = torch.tensor([-20.0, -30.0], dtype=torch.float64)
    asym = -torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi) * (1 - 1 / t ** 2 + 3 / t ** 4)
    assert ((nr.gelu64(t) - asym).abs() / asym.abs()).max() < 1e-4
    big = torch.tensor([-3e38, -7e4, 7e4, 3e38], dtype=torch.float64)
    assert torch.equal(nr.gelu64(big), torch.tensor([-0.0, -0.0, 7e4, 3e38], dtype=torch.float64))
    assert torch.equal(nr.gelu_grad64(big), torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=torch.float64))


def test_spacing16():
    v = torch.tensor([0.0, 1e-9, 2.0 ** -14, 1.0, 1.999, 2.0, 1000.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 0.5], dtype=torch.float64)
    assert torch.equal(nr.spacing16(v, torch.float16), want)
    for dt in (torch.float16, torch.bfloat16):          # against the type itself: the next representable value
        x = torch.tensor([0.37, 1.0, 5.5, 300.0]).to(dt)
        nxt = torch.nextafter(x, torch.full_like(x, float('inf')))
        assert torch.equal(nr.spacing16(x.double(), dt), nxt.double() - x.double())
    assert nr.spacing16(torch.tensor([0.0], dtype=torch.float64), torch.bfloat16).item() == 2.0 ** -133
