"""Every launch class of csrc/rowgemm.hip and csrc/fused_mlp.hip through the C entries: bit-exact where integer arithmetic
makes the result exact, held to the 16-bit floor elsewhere, the fast GELU pointwise.

tests/mlp_ref.py evaluates every operation twice in fp64: with the rounding hook r = identity (the EXACT reference) and with
r = a round trip through the library's 16-bit type at the places where the kernels round (the FLOOR).  16-bit outputs are held
to RMS_MARGIN / ROW_MARGIN times the floor's own error, fp32 statistics to F32_BOUND of the tensor's maximum, the exact cases
bit for bit to the fp64 result converted once; values behind a GELU get the allowances of mlp_ref (the erf GELU of the row
GEMM: tests/NORM_ACT_ERROR_BUDGET.md; the fast GELU of the one-kernel MLP: the two figures of the common.hpp header).  No bound
is fitted to the kernels.  Every case first asserts, through clv_rowgemm_plan / clv_mlp_fused_plan, the launch it was written
for.  Outputs start as NaN inside buffers whose padding columns hold a sentinel and whose rows past M must stay NaN.
Measured figures: tests/MLP_ERROR_BUDGET.md (every case prints them as MLP_BUDGET lines under `pytest -s`)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref as gr                      # noqa: E402
import mlp_ref as mr                       # noqa: E402
import norm_ref as nr                      # noqa: E402
from clover_amd import _lib                # noqa: E402

DEV = 'cuda'
HALF = _lib.half_dtype()
NAN = float('nan')
# kernel error <= margin x floor error, the degenerate-row rule and the fp32 bound: those of tests/test_norm_act_gpu.py.
# None may be raised.
RMS_MARGIN, ROW_MARGIN = 2.0, 4.0
DEGENERATE_ROW = 1e-3
F32_BOUND = 1e-5
ERR_ARG, ERR_UNSUPPORTED = -1, -2
SENT = -7.0                                # padding columns [W, ld) of every 16-bit buffer
TAIL = 32                                  # NaN rows after M
F32_OUT = ('mean', 'rstd')


def ops():
    from clover_amd import ops as o
    return o


def L():
    return _lib.lib()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(t, dtype=None):
    if t is None:
        return None
    t = t.to(DEV)
    return t.to(dtype).contiguous() if dtype is not None else t.contiguous()


def g16(seed, *shape, scale=1.0):
    return (mr.gauss(seed, *shape, device=DEV) * scale).to(HALF)


# ----------------------------------------------------------------------------- guarded buffers
class Mat:
    """A 16-bit matrix [M][W] with row stride ld >= W: columns [W, ld) hold SENT, TAIL rows after M hold NaN.  src = None: an
    output, NaN until the kernel writes it."""

    def __init__(self, M, W, ld, src=None):
        self.M, self.W = M, W
        self.buf = torch.full((M + TAIL, ld), NAN, dtype=HALF, device=DEV)
        self.buf[:, W:] = SENT
        self.view = self.buf[:M, :W]
        if src is not None:
            self.view.copy_(src)
        self.before = self.buf.clone() if src is not None else None

    def check(self, what):
        assert (self.buf[:, self.W:] == SENT).all(), f'{what}: padding columns [W, ld) written'
        assert torch.isnan(self.buf[self.M:, :self.W]).all(), f'{what}: rows past M written'
        if self.before is not None:
            assert torch.equal(self.buf.view(torch.int16), self.before.view(torch.int16)), f'{what}: an operand was written'


def vec32(M):
    return torch.full((M + TAIL,), NAN, dtype=torch.float32, device=DEV)


def same(got, want64, what):
    """bit-exact: a 16-bit device tensor against the fp64 expectation converted once to the 16-bit type"""
    w = want64.to(DEV).to(HALF)
    if not torch.equal(got, w):
        bad = (got != w) | torch.isnan(got)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference '
                             f'({int(torch.isnan(got).sum())} NaN), first at {idx}: got {got[tuple(idx)].item()}, '
                             f'exact {want64[tuple(idx)].item()}')


def within(got, want64, allow, what):
    g = got.double()
    assert torch.isfinite(g).all(), f'{what}: non-finite values (or elements that were never written)'
    frac = ((g - want64).abs() / allow).max().item()
    print(f'MLP_BUDGET | {what} | worst fraction of the allowance {frac:.3f}')
    if frac > 1:
        over = (g - want64).abs() - allow
        idx = over.argmax().item()
        m, n = divmod(idx, got.shape[1])
        raise AssertionError(f'{what}: {int((over > 0).sum())} elements over the allowance, worst at ({m}, {n}): got '
                             f'{g[m, n].item()}, reference {want64[m, n].item()}, allowed {allow[m, n].item():.3e}')


def rms_err(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-300)).item()


def row_err(a, b):
    norm = b.abs().amax(1).clamp_min(DEGENERATE_ROW * b.abs().max()).clamp_min(1e-300)
    return ((a - b).abs().amax(1) / norm).max().item()


def max_err(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _ratio(k, f):
    return k / f if f > 0 else (0.0 if k == 0 else float('inf'))


def hold(case, got, exact, floor):
    """got / exact / floor: dicts of tensors (None entries of `got`: not produced).  16-bit outputs against the floor, mean /
    rstd against F32_BOUND.  Prints, then asserts all at once."""
    bad = []
    for name, g in got.items():
        if g is None:
            continue
        e = exact[name]
        g = g.double()
        assert g.shape == e.shape, (name, g.shape, e.shape)
        assert torch.isfinite(g).all(), f'{case} {name}: non-finite values (or rows that were never written)'
        if name in F32_OUT:
            me = max_err(g, e)
            print(f'MLP_BUDGET | {case} | {name} | fp32 max/max {me:.2e}')
            if me > F32_BOUND:
                bad.append(f'{name}: max error {me:.3e} of the maximum (allowed {F32_BOUND})')
            continue
        f = floor[name]
        fr, kr, fs, ks = rms_err(f, e), rms_err(g, e), row_err(f, e), row_err(g, e)
        print(f'MLP_BUDGET | {case} | {name} | floor rms {fr:.3e} kernel/floor {_ratio(kr, fr):.3f} | floor row {fs:.3e} '
              f'kernel/floor {_ratio(ks, fs):.3f}')
        if kr > RMS_MARGIN * fr:
            bad.append(f'{name}: RMS error {kr:.3e} = {_ratio(kr, fr):.2f} x floor {fr:.3e} (allowed {RMS_MARGIN})')
        if ks > ROW_MARGIN * fs:
            bad.append(f'{name}: row error {ks:.3e} = {_ratio(ks, fs):.2f} x floor {fs:.3e} (allowed {ROW_MARGIN})')
    assert not bad, f'{case}: ' + '; '.join(bad)


# ----------------------------------------------------------------------------- clv_rowgemm, one launch, checked
def rg_launch(c, x, res, wt, bias, pre_in, fac, rps, ldx_pad=0, ldy_pad=0, claim=True):
    """-> dict(y, pre, s, xhat, mean, rstd) (views; None where the mode produces none)"""
    if claim:
        mr.assert_rg(c)
    M, N, K = c.M, c.N, c.K
    std, epi = mr.MODES[c.mode]
    ldx, ldy = K + ldx_pad, N + ldy_pad
    X = Mat(M, K, ldx, dev(x))
    R = Mat(M, K, ldx, dev(res)) if res is not None else None
    S = Mat(M, K, ldx) if res is not None else None
    XH = Mat(M, K, ldx) if std else None
    Y = Mat(M, N, ldy)
    PO = Mat(M, N, ldy) if epi == mr.EPI_GELU else None
    PI = Mat(M, N, ldy, dev(pre_in)) if epi == mr.EPI_GELU_BWD else None
    mean, rstd = (vec32(M), vec32(M)) if std else (None, None)
    wd, bd, xs = dev(wt, HALF), dev(bias, torch.float32), dev(fac, torch.float32)
    b = lambda m: P(m.buf) if m is not None else None      # noqa: E731
    args = [b(X), b(R), b(S), P(mean), P(rstd), b(XH), P(wd), P(bd), b(PI), b(Y), b(PO), M, N, K, ldx, ldy, std, epi, mr.EPS]
    if xs is not None:
        rc = L().clv_rowgemm_xs(*args, P(xs), rps, stream())
    else:
        rc = L().clv_rowgemm(*args, stream())
    torch.cuda.synchronize()
    what = f'{M}x{N}x{K} {c.mode}'
    assert rc == 0, f'{what}: clv_rowgemm = {rc}'
    for m in (X, R, S, XH, Y, PO, PI):
        if m is not None:
            m.check(what)
    if std:
        assert torch.isnan(mean[M:]).all() and torch.isnan(rstd[M:]).all(), f'{what}: statistics written past M'
    v = lambda m: m.view if m is not None else None         # noqa: E731
    return dict(y=Y.view, pre=v(PO), s=v(S), xhat=v(XH), mean=mean[:M] if std else None, rstd=rstd[:M] if std else None)


def rg_exact(c, name, **pads):
    std, epi = mr.MODES[c.mode]
    what = f'{name} {c.M}x{c.N}x{c.K} {c.mode} exact'
    if std:
        gelu = epi == mr.EPI_GELU
        e = mr.std_exact_case(c.M, c.N, c.K, gelu, c.res, c.samples, device=DEV)
        o = rg_launch(c, e.a, e.res, e.wt, e.bias, None, e.fac, e.rps, **pads)
        t, pre = e.t.double().to(DEV), e.acc + e.bias.double().to(DEV)
        same(o['xhat'], t, what + ': xhat')
        if c.res:
            same(o['s'], t, what + ': s')              # (where the factor is 0, a is arbitrary: it must not reach s)
        assert (o['mean'] == 0).all(), f'{what}: the mean of a +-1 row is exactly 0'
        assert ((o['rstd'].double() - (1 + mr.EPS) ** -0.5).abs() <= F32_BOUND).all(), what + ': rstd'
        if gelu:
            same(o['pre'], pre, what + ': pre_out')
            within(o['y'], nr.gelu64(pre), mr.erf_gelu_allow(pre), what + ': y')
        else:
            same(o['y'], pre, what + ': y')
        return
    e = gr.exact_case(c.M, c.N, c.K, gelu=epi == mr.EPI_GELU_BWD, device=DEV)
    pre = e.acc + e.bias.double().to(DEV)
    if epi == mr.EPI_NONE:
        o = rg_launch(c, e.a, None, e.b, e.bias, None, None, 1, **pads)
        same(o['y'], pre, what + ': y')
    else:
        o = rg_launch(c, e.a, None, e.b, e.bias, e.aux, None, 1, **pads)
        aux = e.aux.double().to(DEV)
        within(o['y'], pre * nr.gelu_grad64(aux), mr.erf_gelu_grad_allow(aux) * pre.abs() + 1e-300, what + ': y')


def rg_inputs(c, seed=0):
    """Gaussian 16-bit operands on the device; fp32 bias, left unrounded"""
    M, N, K = c.M, c.N, c.K
    s = 7919 * M + 31 * N + K + 1000003 * seed
    x, wt = g16(s + 1, M, K), g16(s + 2, N, K, scale=K ** -0.5)
    res = g16(s + 3, M, K) if c.res else None
    bias = mr.gauss(s + 4, N, device=DEV) * 0.5
    pre_in = g16(s + 5, M, N) if c.mode == 'dgelu' else None
    fac, rps, k = None, 1, None
    if c.samples:
        fac, rps = mr.factors(c.samples).to(DEV), M // c.samples
        k = fac.repeat_interleave(rps)
    return x, res, wt, bias, pre_in, fac, rps, k


def rg_refs(c, x, res, wt, bias, pre_in, k):
    std, epi = mr.MODES[c.mode]
    if std:
        fn = lambda r: mr.by_rows(lambda x_, r_, k_, *w: mr.rowgemm_std(x_, r_, k_, *w, epi == mr.EPI_GELU, r), [x, res, k], [wt, bias])   # noqa: E731
    else:
        fn = lambda r: mr.by_rows(lambda x_, p_, *w: mr.rowgemm_plain(x_, *w, p_, r), [x, pre_in], [wt, bias])   # noqa: E731
    return fn(nr.ident), fn(gr.round16)


def rg_gauss(c, name, **pads):
    x, res, wt, bias, pre_in, fac, rps, k = rg_inputs(c)
    o = rg_launch(c, x, res, wt, bias, pre_in, fac, rps, **pads)
    exact, floor = rg_refs(c, x, res, wt, bias, pre_in, k)
    hold(f'{name} {c.M}x{c.N}x{c.K} {c.mode}', o, exact, floor)
    if k is not None and c.res:
        dead = k == 0
        assert torch.equal(o['s'][dead], dev(res)[dead]), 'a sample of factor 0: s must be the residual, bit for bit'


@pytest.mark.parametrize('kind', ['exact', 'gauss'])
@pytest.mark.parametrize('K,mode', list(mr.SMALL))
def test_rowgemm_every_instantiation(K, mode, kind):
    """the 26 instantiations rowgemm_impl reaches, each at M = 1, 17 and 2069 with a partial last column tile"""
    for M in mr.SMALL_MS:
        (rg_exact if kind == 'exact' else rg_gauss)(mr.small_case(K, mode, M), 'small')


@pytest.mark.parametrize('kind', ['exact', 'gauss'])
@pytest.mark.parametrize('name', list(mr.TRIPS))
def test_rowgemm_second_trip(name, kind):
    """every (prologue, epilogue, waves) class with a second row tile per wave: the loop-carried staging tiles, the wave
    barriers between trips, the XCD swizzle with whole groups of 8 row slices"""
    c = mr.TRIPS[name]
    assert c.claim.trips >= 2
    (rg_exact if kind == 'exact' else rg_gauss)(c, name)


@pytest.mark.parametrize('mode', list(mr.STRIDED))
def test_rowgemm_row_strides(mode):
    """ldx = K + 8, ldy = N + 8: the padding columns of x / res / s / xhat and of y / pre_in / pre_out keep their sentinel"""
    c = mr.STRIDED[mode]
    rg_exact(c, 'strided', ldx_pad=8, ldy_pad=8)
    rg_gauss(c, 'strided', ldx_pad=8, ldy_pad=8)


@pytest.mark.parametrize('mode', ['std', 'std_gelu'])
def test_rowgemm_prologue_outputs_written_once(mode):
    """mean, rstd, s and xhat_out are written by the first column tile only: a launch with ny = 3 gives, bit for bit, those of
    the ny = 1 launch on the first 64 columns (and the same y there)."""
    c3 = mr.small_case(96, mode, 2069)
    assert c3.claim.ny == 3
    c1 = c3._replace(N=64, claim=c3.claim._replace(ny=1))
    x, res, wt, bias, pre_in, fac, rps, k = rg_inputs(c3)
    o3 = rg_launch(c3, x, res, wt, bias, None, fac, rps)
    o1 = rg_launch(c1, x, res, wt[:64].contiguous(), bias[:64].contiguous(), None, fac, rps)
    for name in ('mean', 'rstd', 's', 'xhat'):
        assert torch.isfinite(o3[name].float()).all() and torch.equal(o3[name], o1[name]), name
    assert torch.equal(o3['y'][:, :64], o1['y'])
    if mode == 'std_gelu':
        assert torch.equal(o3['pre'][:, :64], o1['pre'])


def test_rowgemm_error_codes():
    M, N, K = 32, 64, 96
    x, res, s, y, pre = (Mat(M, W, W, g16(i, M, W)) for i, W in enumerate((K, K, K, N, N)))
    out = Mat(M, N, N)
    wt, bias, mean, rstd = g16(9, N, 768), torch.zeros(N, device=DEV), vec32(M), vec32(M)
    xs = torch.ones(1, device=DEV)

    def call(K_=K, N_=N, res_=None, s_=None, std=0, epi=0, pre_in=None, pre_out=None, ldx=None, ldy=None, xscale=None):
        a = [P(x.buf), P(res_), P(s_), P(mean), P(rstd), None, P(wt), P(bias), P(pre_in), P(out.buf), P(pre_out), M, N_, K_,
             K_ if ldx is None else ldx, N_ if ldy is None else ldy, std, epi, mr.EPS]
        return L().clv_rowgemm_xs(*a, P(xscale), M, stream()) if xscale is not None else L().clv_rowgemm(*a, stream())

    assert call(K_=160) == ERR_ARG and call(K_=64) == ERR_ARG                  # unsupported K
    assert call(K_=288, std=1) == ERR_ARG                                      # (standardise needs K <= 256)
    assert call(N_=60) == ERR_ARG                                              # N % 8
    assert call(res_=res.buf, s_=s.buf) == ERR_UNSUPPORTED                      # res without standardise
    assert call(res_=res.buf, std=1) == ERR_ARG                                # res without sum_out
    assert call(std=1, xscale=xs) == ERR_ARG                                   # xscale without res
    assert call(epi=2) == ERR_ARG and call(std=1, epi=1) == ERR_ARG            # missing pre_in / pre_out
    assert call(ldx=K - 8) == ERR_ARG and call(ldy=N - 8) == ERR_ARG           # ld < width
    assert call(ldx=K + 4) == ERR_ARG and call(ldy=N + 4) == ERR_ARG           # ld % 8
    assert call(epi=1, pre_out=pre.buf) == ERR_UNSUPPORTED and call(std=1, epi=2, pre_in=pre.buf) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(out.buf).all() and torch.isnan(mean).all(), 'a refused call wrote to its outputs'
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out.view.float()).all()


# ----------------------------------------------------------------------------- clv_mlp_fused_fwd / _bwd
def rows16(M, W, src=None):
    """contiguous [M][W] 16-bit rows followed by TAIL NaN rows -> (buffer, view)"""
    buf = torch.full((M + TAIL, W), NAN, dtype=HALF, device=DEV)
    if src is not None:
        buf[:M].copy_(src)
    return buf, buf[:M]


def tails_nan(bufs, M, what):
    for name, b in bufs.items():
        if b is not None:
            assert torch.isnan(b[M:]).all(), f'{what}: {name} written past M'


def fm_fwd(M, a, res, fac, rps, w1f, b1f, w2, b2):
    A, R = rows16(M, mr.FM_C, dev(a))[0], (rows16(M, mr.FM_C, dev(res))[0] if res is not None else None)
    S = rows16(M, mr.FM_C)[0] if res is not None else None
    O, mean, rstd = rows16(M, mr.FM_C)[0], vec32(M), vec32(M)
    xs = dev(fac, torch.float32)
    keep = [dev(w1f, HALF), dev(b1f, torch.float32), dev(w2, HALF), dev(b2, torch.float32)]
    rc = L().clv_mlp_fused_fwd(P(A), P(R), P(S), P(mean), P(rstd), P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), P(O), M,
                               mr.FM_C, mr.FM_H, mr.EPS, P(xs), rps, stream())
    torch.cuda.synchronize()
    assert rc == 0, f'clv_mlp_fused_fwd = {rc}'
    tails_nan(dict(sum_out=S, out=O, mean=mean, rstd=rstd), M, f'one-kernel forward, M = {M}')
    return dict(out=O[:M], s=S[:M] if S is not None else None, mean=mean[:M], rstd=rstd[:M])


def fm_bwd(M, ts, mean, rstd, dout, dsum, fac, rps, w1f, b1f, w2, want_dres):
    T, DO = rows16(M, mr.FM_C, dev(ts))[0], rows16(M, mr.FM_C, dev(dout))[0]
    DS = rows16(M, mr.FM_C, dev(dsum))[0] if dsum is not None else None
    DA, XH = rows16(M, mr.FM_C)[0], rows16(M, mr.FM_C)[0]
    DR = rows16(M, mr.FM_C)[0] if want_dres else None
    ACT, DP = rows16(M, mr.FM_H)[0], rows16(M, mr.FM_H)[0]
    mu, rs = vec32(M), vec32(M)
    mu[:M], rs[:M] = dev(mean, torch.float32), dev(rstd, torch.float32)
    xs = dev(fac, torch.float32)
    keep = [dev(w1f, HALF), dev(b1f, torch.float32), dev(w2, HALF).t().contiguous()]
    rc = L().clv_mlp_fused_bwd(P(T), P(mu), P(rs), P(DO), P(DS), P(keep[0]), P(keep[1]), P(keep[2]), P(DA), P(DR), P(ACT),
                               P(DP), P(XH), M, mr.FM_C, mr.FM_H, P(xs), rps, stream())
    torch.cuda.synchronize()
    assert rc == 0, f'clv_mlp_fused_bwd = {rc}'
    tails_nan(dict(da=DA, dres=DR, act=ACT, dpre=DP, xhat=XH), M, f'one-kernel backward, M = {M}')
    return dict(da=DA[:M], dres=DR[:M] if want_dres else None, act=ACT[:M], dpre=DP[:M], xhat=XH[:M])


def fm_weights(seed=0):
    w1f, b1f = g16(seed + 153, mr.FM_H, mr.FM_C, scale=0.12), mr.gauss(seed + 154, mr.FM_H, device=DEV) * 0.1
    w2, b2 = g16(seed + 155, mr.FM_C, mr.FM_H, scale=0.06), mr.gauss(seed + 156, mr.FM_C, device=DEV) * 0.1
    return w1f, b1f, w2, b2


def fm_factors(M, variant, exact=False):
    if variant != 'res_xscale':
        return None, 1, None
    B = mr.samples_of(M)
    fac = mr.factors(B, exact).to(DEV)
    return fac, M // B, fac.repeat_interleave(M // B)


def fwd_refs(a, res, k, w):
    fn = lambda r: mr.by_rows(lambda a_, r_, k_, *w_: mr.mlp_fwd(a_, r_, k_, *w_, r), [a, res, k], list(w))      # noqa: E731
    return fn(nr.ident), fn(gr.round16)


def bwd_refs(ts, mean, rstd, dout, dsum, k, w, want_dres):
    fn = lambda r: mr.by_rows(lambda t_, m_, s_, d_, ds_, k_, *w_: mr.mlp_bwd(t_, m_, s_, d_, ds_, k_, *w_, r, want_dres),      # noqa: E731
                              [ts, mean, rstd, dout, dsum, k], list(w))
    return fn(nr.ident), fn(gr.round16)


@pytest.mark.parametrize('variant', mr.FM_VARIANTS)
@pytest.mark.parametrize('M', list(mr.FM_CASES))
def test_one_kernel_mlp_to_the_floor(M, variant):
    """Forward out / s / statistics, then the backward on the REFERENCE's own stored stream and statistics (converted to fp32),
    once with and once without the stream's gradient and dres."""
    mr.assert_fm(M)
    case = f'one-kernel M={M} {variant}'
    w1f, b1f, w2, b2 = fm_weights()
    a, res = g16(M + 1, M, mr.FM_C), (g16(M + 2, M, mr.FM_C) if variant != 'plain' else None)
    dout, dsum = g16(M + 3, M, mr.FM_C), g16(M + 4, M, mr.FM_C)
    fac, rps, k = fm_factors(M, variant)
    got = fm_fwd(M, a, res, fac, rps, w1f, b1f, w2, b2)
    exact, floor = fwd_refs(a, res, k, (w1f, b1f, w2, b2))
    hold(case + ' fwd', got, exact, floor)
    ts = floor['s'].to(HALF) if res is not None else a
    mean32, rstd32 = exact['mean'].float(), exact['rstd'].float()
    for with_extra in (True, False):
        ds = dsum if with_extra else None
        gb = fm_bwd(M, ts, mean32, rstd32, dout, ds, fac, rps, w1f, b1f, w2, want_dres=with_extra)
        be, bf = bwd_refs(ts, mean32, rstd32, dout, ds, k, (w1f, b1f, w2), with_extra)
        hold(f'{case} bwd{" +dsum +dres" if with_extra else ""}', gb, be, bf)
        if k is not None and (k == 0).any():
            assert (gb['da'][k == 0] == 0).all(), f'{case}: a sample of factor 0 got a gradient into its branch'


@pytest.mark.parametrize('variant', mr.FM_VARIANTS)
@pytest.mark.parametrize('M', list(mr.FM_CASES))
def test_one_kernel_mlp_exact(M, variant):
    """+-1 rows: s and xhat bit for bit, mean == 0; act within the fast-GELU allowance of the exact pre-activation, dpre within
    |dact| times the fast-GELU' allowance (dact = dout W2 is an exact integer)."""
    mr.assert_fm(M)
    what = f'one-kernel M={M} {variant} exact'
    e = mr.fm_exact_case(M, variant, device=DEV)
    b2 = torch.arange(mr.FM_C).float() % 5 - 2
    f = fm_fwd(M, e.a, e.res, e.fac, e.rps, e.w1f, e.b1f, e.w2, b2)
    t = e.t.double().to(DEV)
    assert (f['mean'] == 0).all(), what + ': mean'
    assert ((f['rstd'].double() - (1 + mr.EPS) ** -0.5).abs() <= F32_BOUND).all(), what + ': rstd'
    assert torch.isfinite(f['out'].float()).all()
    if e.res is not None:
        same(f['s'], t, what + ': s')
    rstd = torch.full((M,), (1 + mr.EPS) ** -0.5)
    b = fm_bwd(M, e.t.to(HALF), torch.zeros(M), rstd, e.dout, None, e.fac, e.rps, e.w1f, e.b1f, e.w2, want_dres=True)
    same(b['xhat'], t, what + ': xhat_out')
    within(b['act'], nr.gelu64(e.h), mr.fast_gelu_allow(e.h), what + ': act_out')
    within(b['dpre'], e.dact * nr.gelu_grad64(e.h), e.dact.abs() * mr.fast_gelu_grad_allow(e.h) + 1e-300, what + ': dpre_out')
    assert torch.isfinite(b['da'].float()).all() and torch.isfinite(b['dres'].float()).all()
    if e.k is not None and (e.k == 0).any():
        assert (b['da'][e.k.to(DEV) == 0] == 0).all()


@pytest.mark.parametrize('with_res', [False, True])
def test_one_kernel_mlp_through_autograd(with_res):
    """ops.fused_mlp at M = 69643 = 7 x 9949 (the prefetched full group): out, s, d a and d r to the floor — the saved-tensor
    plumbing between the two kernels (the stored stream, the statistics, the folded weights, the per-sample factors)."""
    B, rps = 7, 9949
    M = B * rps
    mr.assert_fm(M)
    a, r = g16(501, B, rps, mr.FM_C).requires_grad_(), (g16(502, B, rps, mr.FM_C).requires_grad_() if with_res else None)
    G = dict(g=1 + 0.1 * mr.gauss(503, mr.FM_C, device=DEV), b=0.1 * mr.gauss(504, mr.FM_C, device=DEV),
             w1=mr.gauss(505, mr.FM_H, mr.FM_C, device=DEV) * 0.12, b1=mr.gauss(506, mr.FM_H, device=DEV) * 0.1,
             w2=mr.gauss(507, mr.FM_C, mr.FM_H, device=DEV) * 0.06, b2=mr.gauss(508, mr.FM_C, device=DEV) * 0.1)
    G = {n: v.requires_grad_() for n, v in G.items()}
    fac = mr.factors(B).to(DEV) if with_res else None
    dout, dsum = g16(509, B, rps, mr.FM_C), g16(510, B, rps, mr.FM_C)
    assert ops().mlp_fused_ok(a.detach().view(M, mr.FM_C), mr.FM_H), 'the one-kernel path is not taken'
    m, s2 = ops().fused_mlp(a, r, G['g'], G['b'], G['w1'], G['b1'], G['w2'], G['b2'], x_scale=fac)
    if with_res:
        torch.autograd.backward([m, s2], [dout, dsum])
    else:
        assert s2 is None
        torch.autograd.backward([m], [dout])
    torch.cuda.synchronize()
    # the reference runs on the operands the kernels were given: the folded fc1 of ops.fold_layernorm, W2 in 16 bits
    w1f, b1f = ops().fold_layernorm(G['w1'], G['b1'], G['g'], G['b'])
    w = (w1f, b1f, G['w2'].detach().to(HALF), G['b2'].detach())
    a2, r2 = a.detach().view(M, -1), (r.detach().view(M, -1) if with_res else None)
    k = fac.repeat_interleave(rps) if with_res else None
    exact, floor = fwd_refs(a2, r2, k, w)
    got = dict(out=m.detach().view(M, -1), s=s2.detach().view(M, -1) if with_res else None)
    hold(f'autograd M={M} res={with_res} fwd', got, exact, floor)
    ds2 = dsum.view(M, -1) if with_res else None
    be = mr.by_rows(lambda t_, m_, s_, d_, ds_, k_, *w_: mr.mlp_bwd(t_, m_, s_, d_, ds_, k_, *w_, nr.ident),
                    [exact['s'] if with_res else a2, exact['mean'], exact['rstd'], dout.view(M, -1), ds2, k], list(w[:3]))
    bf = mr.by_rows(lambda t_, m_, s_, d_, ds_, k_, *w_: mr.mlp_bwd(t_, m_, s_, d_, ds_, k_, *w_, gr.round16),
                    [floor['s'] if with_res else a2, exact['mean'], exact['rstd'], dout.view(M, -1), ds2, k], list(w[:3]))
    gb = dict(da=a.grad.view(M, -1), dres=r.grad.view(M, -1) if with_res else None)
    hold(f'autograd M={M} res={with_res} bwd', gb, be, bf)
    if with_res:
        assert (a.grad[1] == 0).all()
    for n, v in G.items():
        assert v.grad is not None and torch.isfinite(v.grad).all(), n


# ----------------------------------------------------------------------------- the fast GELU, pointwise
def _rows_identical(t, what):
    assert torch.equal(t.view(torch.int16), t[:1].expand_as(t).contiguous().view(torch.int16)), f'{what}: rows differ'


@pytest.mark.parametrize('M', mr.GELU_SWEEP_MS)
def test_fast_gelu_pointwise_forward(M):
    """W1f = 0 makes the pre-activation of every token b1f; W2 = a selection of 96 hidden units and b2 = 0 make out their
    16-bit GELU: gelu_fast2 at 12 672 points through fm_fwd_group<1> (M = 16) and fm_fwd_group<2> (M = 8192)."""
    p = mr.assert_fm(M)
    assert (p.tiles_max == 1) if M == 16 else (p.tiles_min == 2 and p.half_group == 0)
    pts = mr.gelu_sweep_points().to(DEV)
    w1f, b2 = torch.zeros(mr.FM_H, mr.FM_C, dtype=HALF, device=DEV), torch.zeros(mr.FM_C, device=DEV)
    sel = []
    for q in range(4):
        w2 = torch.zeros(mr.FM_C, mr.FM_H, dtype=HALF, device=DEV)
        w2[torch.arange(mr.FM_C), torch.arange(mr.FM_C) + mr.FM_C * q] = 1
        sel.append(w2)
    a = g16(77, M, mr.FM_C)
    out = torch.full((M, mr.FM_C), NAN, dtype=HALF, device=DEV)
    mean, rstd = vec32(M), vec32(M)
    got = torch.empty_like(pts, dtype=HALF)
    for i in range(pts.shape[0]):
        for q in range(4):
            out.fill_(NAN)
            rc = L().clv_mlp_fused_fwd(P(a), None, None, P(mean), P(rstd), P(w1f), P(pts[i]), P(sel[q]), P(b2), P(out), M, mr.FM_C,
                                       mr.FM_H, mr.EPS, None, 1, stream())
            assert rc == 0
            _rows_identical(out, f'M={M} launch {i}.{q}')
            got[i, mr.FM_C * q:mr.FM_C * (q + 1)] = out[0]
    x = pts.double()
    within(got, nr.gelu64(x), mr.fast_gelu_allow(x), f'fast GELU forward M={M}')


@pytest.mark.parametrize('M', mr.GELU_SWEEP_MS)
def test_fast_gelu_pointwise_backward(M):
    """dout = e_0 and W2^T[:, 0] = 1 make dact = 1: act_out and dpre_out are the 16-bit gelu_fast_both2 of b1f."""
    mr.assert_fm(M)
    pts = mr.gelu_sweep_points().to(DEV)
    w1f = torch.zeros(mr.FM_H, mr.FM_C, dtype=HALF, device=DEV)
    w2t = torch.zeros(mr.FM_H, mr.FM_C, dtype=HALF, device=DEV)
    w2t[:, 0] = 1
    ts, dout = torch.zeros(M, mr.FM_C, dtype=HALF, device=DEV), torch.zeros(M, mr.FM_C, dtype=HALF, device=DEV)
    dout[:, 0] = 1
    mean, rstd = torch.zeros(M, device=DEV), torch.ones(M, device=DEV)
    da = torch.empty(M, mr.FM_C, dtype=HALF, device=DEV)
    act = torch.full((M, mr.FM_H), NAN, dtype=HALF, device=DEV)
    dpre = act.clone()
    ga, gd = torch.empty_like(pts, dtype=HALF), torch.empty_like(pts, dtype=HALF)
    for i in range(pts.shape[0]):
        act.fill_(NAN)
        dpre.fill_(NAN)
        rc = L().clv_mlp_fused_bwd(P(ts), P(mean), P(rstd), P(dout), None, P(w1f), P(pts[i]), P(w2t), P(da), None, P(act), P(dpre),
                                   None, M, mr.FM_C, mr.FM_H, None, 1, stream())
        assert rc == 0
        _rows_identical(act, f'M={M} launch {i}: act')
        _rows_identical(dpre, f'M={M} launch {i}: dpre')
        ga[i], gd[i] = act[0], dpre[0]
    x = pts.double()
    within(ga, nr.gelu64(x), mr.fast_gelu_allow(x), f'fast GELU backward act M={M}')
    within(gd, nr.gelu_grad64(x), mr.fast_gelu_grad_allow(x), f"fast GELU' M={M}")


def test_one_kernel_error_codes():
    t = g16(1, 16, mr.FM_C)
    q = _lib.ClvMlpFusedPlan()
    assert L().clv_mlp_fused_plan(0, q) == ERR_ARG
    rc = L().clv_mlp_fused_fwd(P(t), None, None, P(t), P(t), P(t), P(t), P(t), None, P(t), 16, 128, 384, mr.EPS, None, 1, stream())
    assert rc == ERR_UNSUPPORTED
    rc = L().clv_mlp_fused_fwd(P(t), P(t), None, P(t), P(t), P(t), P(t), P(t), None, P(t), 16, 96, 384, mr.EPS, None, 1, stream())
    assert rc == ERR_ARG                                                       # res without sum_out
    rc = L().clv_mlp_fused_fwd(P(t), None, None, P(t), P(t), P(t), P(t), P(t), None, P(t), 16, 96, 384, mr.EPS, P(t), 4, stream())
    assert rc == ERR_ARG                                                       # xscale without res
