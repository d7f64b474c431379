"""References, input generators and launch claims for the tests of csrc/rowgemm.hip and csrc/fused_mlp.hip
(tests/test_mlp_ref_cpu.py, tests/test_mlp_gpu.py).  Plain torch in fp64 on any device; the only library calls are the HOST
entries clv_rowgemm_plan / clv_mlp_fused_plan.

Every reference takes a rounding hook r, as norm_ref.ln_core does: r = nr.ident gives the EXACT reference, r = gr.round16 (a
round trip through the library's 16-bit type) the FLOOR — what the element type alone costs.  The floor rounds where the
kernels round and nowhere else (tests/MLP_ERROR_BUDGET.md names the kernel line behind each rounding).

Exactness.  The plain row GEMM takes the ternary operands of gemm_ref.exact_case.  The standardised paths (row GEMM with the
LayerNorm prologue, the one-kernel MLP) take rows that are permutations of K/2 values +1 and K/2 values -1: the mean is exactly 0,
(t - mean) rstd = +-(1 + eps)^-1/2 rounds to +-1 in both 16-bit types, and with ternary weights every product sum is exact.
The caps of gemm_ref.check_caps are asserted on the inputs and the reference alone.

Claims.  Every case names the launch it was written for as a literal record; assert_rg / assert_fm compare it with what the
library's host entries say, and the launches dispatch on the same records."""
import functools
from typing import NamedTuple, Optional

import torch

import gemm_ref as gr
import norm_ref as nr
from clover_amd import _lib

HALF = gr.HALF
EPS = 1e-5
EPI_NONE, EPI_GELU, EPI_GELU_BWD = 0, 1, 2
# mode -> (standardise, epilogue): the four (prologue, epilogue) pairs dispatch_rg of rowgemm.hip knows
MODES = {'plain': (0, EPI_NONE), 'dgelu': (0, EPI_GELU_BWD), 'std': (1, EPI_NONE), 'std_gelu': (1, EPI_GELU)}
KS_ALL = (96, 128, 192, 256, 288, 384, 512, 576, 768)
KS_STD = (96, 128, 192, 256)
# the fast GELU of the one-kernel MLP: the two figures of the common.hpp header (|u (h - exact)|, |h - exact|)
FAST_GELU_ABS, FAST_GELU_GRAD_ABS = 3.3e-6, 2.6e-5
FM_C, FM_H = 96, 384
FACTORS = (1.25, 0.0, 0.5, 1.0, 0.75, 1.5, 0.25)        # per-sample DropPath factors, cycled; the exact cases use 1 / 0
FACTORS_EXACT = (1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0)


# ----------------------------------------------------------------------------------------------- launch claims
class RgPlan(NamedTuple):
    TN: int                     # columns of the weight tile
    waves: int                  # per workgroup
    ny: int                     # column tiles
    gx: int                     # persistent row slices
    lds: int                    # bytes
    trips: int                  # 16-row tiles of the busiest wave


class FmPlan(NamedTuple):
    grid: int
    tiles_min: int
    tiles_max: int
    trips: int                  # groups (two tiles) per wave in the fullest workgroup; >= 2: the forward prefetches
    half_group: int             # some workgroup has an odd tile count


def rg_plan(M, N, K, mode):
    p = _lib.ClvRowgemmPlan()
    rc = _lib.lib().clv_rowgemm_plan(M, N, K, *MODES[mode], p)
    assert rc == 0, f'clv_rowgemm_plan({M}, {N}, {K}, {mode}) = {rc}'
    return RgPlan(p.TN, p.waves, p.ny, p.gx, p.lds_bytes, p.trips)


def fm_plan(M):
    p = _lib.ClvMlpFusedPlan()
    rc = _lib.lib().clv_mlp_fused_plan(M, p)
    assert rc == 0, f'clv_mlp_fused_plan({M}) = {rc}'
    return FmPlan(p.grid, p.tiles_min, p.tiles_max, p.trips, p.half_group)


class RgCase(NamedTuple):
    M: int
    N: int
    K: int
    mode: str
    claim: RgPlan
    res: bool = False           # residual operand (standardised modes)
    samples: int = 0            # > 0: xscale with M / samples rows per sample
    note: str = ''


# One small ragged case per instantiation rowgemm_impl can reach (26), at M = 1, 17 and 2069 with N = 136 (the last column
# tile is 8 wide).  (K, mode) -> (TN, waves, ny, lds, gx at M = 2069); gx = 1 at M = 1 and 17, trips = 1 throughout.
SMALL_N = 136
SMALL_MS = (1, 17, 2064 + 5)
SMALL = {
    (96, 'plain'): (64, 4, 3, 22784, 33), (96, 'dgelu'): (64, 8, 3, 50432, 17),
    (96, 'std'): (64, 8, 3, 32000, 17), (96, 'std_gelu'): (64, 8, 3, 50432, 17),
    (128, 'plain'): (64, 4, 3, 26880, 33), (128, 'dgelu'): (64, 8, 3, 54528, 17),
    (128, 'std'): (64, 4, 3, 26880, 33), (128, 'std_gelu'): (64, 4, 3, 36096, 33),
    (192, 'plain'): (128, 12, 2, 103936, 11), (192, 'dgelu'): (128, 12, 2, 156160, 11),
    (192, 'std'): (128, 12, 2, 103936, 11), (192, 'std_gelu'): (128, 12, 2, 156160, 11),
    (256, 'plain'): (128, 12, 2, 120320, 11), (256, 'dgelu'): (128, 8, 2, 137728, 17),
    (256, 'std'): (128, 12, 2, 120320, 11), (256, 'std_gelu'): (128, 8, 2, 137728, 17),
    (288, 'plain'): (128, 8, 2, 111104, 17), (288, 'dgelu'): (128, 8, 2, 145920, 17),
    (384, 'plain'): (128, 8, 2, 135680, 17), (384, 'dgelu'): (128, 4, 2, 135680, 33),
    (512, 'plain'): (64, 4, 3, 76032, 33), (512, 'dgelu'): (64, 4, 3, 85248, 33),
    (576, 'plain'): (64, 4, 3, 84224, 33), (576, 'dgelu'): (64, 4, 3, 93440, 33),
    (768, 'plain'): (64, 4, 3, 108800, 33), (768, 'dgelu'): (64, 4, 3, 118016, 33),
}


def small_case(K, mode, M):
    TN, waves, ny, lds, gx = SMALL[(K, mode)]
    std = bool(MODES[mode][0])
    # the standardised ones: M = 1 bare, M = 17 with a residual, M = 2069 (a prime: one row per sample) with a residual and
    # per-sample factors
    return RgCase(M, SMALL_N, K, mode, RgPlan(TN, waves, ny, gx if M > 17 else 1, lds, 1), res=std and M >= 17,
                  samples=M if (std and M > 17) else 0)


# Every (prologue, epilogue, waves) class with trips = 2 and a ragged last tile (rows, columns or both).  Two classes, (std, 4
# waves) and (dgelu, 12 waves), are reached only through the last two rows.
TRIPS = {
    'plain-w4-k96': RgCase(20001, 288, 96, 'plain', RgPlan(64, 4, 5, 307, 22784, 2)),
    'dgelu-w8-k96': RgCase(33000, 384, 96, 'dgelu', RgPlan(64, 8, 6, 256, 50432, 2)),
    'dgelu-w8-k128': RgCase(33000, 384, 128, 'dgelu', RgPlan(64, 8, 6, 256, 54528, 2)),
    'std-w8-k96': RgCase(33000, 392, 96, 'std', RgPlan(64, 8, 7, 256, 32000, 2)),
    'std_gelu-w8-k96': RgCase(33000, 384, 96, 'std_gelu', RgPlan(64, 8, 6, 256, 50432, 2), res=True, samples=8,
                              note='4125 rows per sample: not a multiple of 16; sample 1 has factor 0'),
    'std_gelu-w4-k128': RgCase(16500, 392, 128, 'std_gelu', RgPlan(64, 4, 7, 256, 36096, 2)),
    'plain-w12-k192': RgCase(24600, 200, 192, 'plain', RgPlan(128, 12, 2, 128, 103936, 2)),
    'std-w12-k192': RgCase(24600, 200, 192, 'std', RgPlan(128, 12, 2, 128, 103936, 2), res=True),
    'std_gelu-w12-k192': RgCase(50000, 776, 192, 'std_gelu', RgPlan(128, 12, 7, 256, 156160, 2)),
    'plain-w8-k288': RgCase(33000, 96, 288, 'plain', RgPlan(128, 8, 1, 256, 111104, 2)),
    'plain-w8-k384': RgCase(33000, 96, 384, 'plain', RgPlan(128, 8, 1, 256, 135680, 2)),
    'dgelu-w4-k384': RgCase(16500, 776, 384, 'dgelu', RgPlan(128, 4, 7, 256, 135680, 2)),
    'plain-w4-k768': RgCase(5600, 136, 768, 'plain', RgPlan(64, 4, 3, 86, 108800, 2)),
    'dgelu-w4-k576': RgCase(16500, 392, 576, 'dgelu', RgPlan(64, 4, 7, 256, 93440, 2)),
    'std-w4-k128': RgCase(16500, 392, 128, 'std', RgPlan(64, 4, 7, 256, 26880, 2)),
    'dgelu-w12-k192': RgCase(49999, 776, 192, 'dgelu', RgPlan(128, 12, 7, 256, 156160, 2)),
}
# one ldx = K + 8 / ldy = N + 8 launch per epilogue
STRIDED = {'plain': small_case(288, 'plain', 2069), 'dgelu': small_case(128, 'dgelu', 2069),
           'std': small_case(192, 'std', 2069), 'std_gelu': small_case(96, 'std_gelu', 2069)}


def assert_rg(c):
    got = rg_plan(c.M, c.N, c.K, c.mode)
    assert got == c.claim, f'{c.M}x{c.N}x{c.K} {c.mode}: the launch moved off the path this case claims: {got} (claimed {c.claim})'
    return c


# M of the one-kernel MLP -> claim
FM_CASES = {
    1: FmPlan(1, 1, 1, 1, 1),           # one tile per workgroup: the half-group body only
    16: FmPlan(1, 1, 1, 1, 1),
    17: FmPlan(2, 1, 1, 1, 1),
    4100: FmPlan(256, 1, 2, 1, 1),      # 257 tiles: the last workgroup has two, the partial tile is the second of a full group
    8192: FmPlan(256, 2, 2, 1, 0),      # all full groups
    12281: FmPlan(256, 3, 3, 1, 1),     # a full group plus a half group, everywhere
    65550: FmPlan(256, 16, 17, 2, 1),   # 4097 tiles: one workgroup has 17: wave 0 prefetches a HALF group
    69643: FmPlan(256, 17, 18, 2, 1),   # 4353 tiles: one workgroup has 18: wave 0 prefetches a FULL group
}
FM_VARIANTS = ('plain', 'res', 'res_xscale')
# the pointwise GELU sweep: the half-group body, and the smallest M at which every workgroup runs full groups only (with
# M <= 4096 the grid is one tile per workgroup, so M = 32 would run the half-group body twice)
GELU_SWEEP_MS = (16, 8192)


def assert_fm(M):
    got = fm_plan(M)
    assert got == FM_CASES[M], f'one-kernel MLP, M = {M}: {got} (claimed {FM_CASES[M]})'
    return got


def samples_of(M):
    """B of the xscale variant: the largest divisor of M that is <= 8, or M itself (one row per sample) when there is none."""
    for b in range(8, 1, -1):
        if M % b == 0:
            return b
    return M


def factors(B, exact=False):
    f = FACTORS_EXACT if exact else FACTORS
    return torch.tensor([f[i % len(f)] for i in range(B)], dtype=torch.float32)


# ----------------------------------------------------------------------------------------------- references
def _d(t, like):
    return None if t is None else t.to(like.device).double()


def _stream(a, res, k):
    """t = a k + res in fp64; k: per-row factor [M] or None"""
    t = a.double()
    if k is not None:
        t = t * _d(k, a)[:, None]
    if res is not None:
        t = t + res.double()
    return t


def _stats(t, eps):
    mu = t.mean(-1, keepdim=True)
    rstd = ((t - mu).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    return mu, rstd


def rowgemm_std(a, res, k, wt, bias, gelu, r, eps=EPS):
    """clv_rowgemm with standardise: -> dict(y, pre (GELU only), s, mean, rstd, xhat).  The statistics come from the
    UNROUNDED t; bias is fp32 and enters unrounded; GELU is taken from the unrounded pre-activation."""
    t = _stream(a, res, k)
    mu, rstd = _stats(t, eps)
    xhat = r((t - mu) * rstd)
    pre = xhat @ _d(wt, a).t() + _d(bias, a)
    out = dict(s=r(t), mean=mu.squeeze(-1), rstd=rstd.squeeze(-1), xhat=xhat, pre_exact=pre)
    if gelu:
        out.update(pre=r(pre), y=r(nr.gelu64(pre)))
    else:
        out.update(y=r(pre))
    return out


def rowgemm_plain(x, wt, bias, pre_in, r):
    """clv_rowgemm without prologue: y = r(x Wt^T + bias), times gelu'(pre_in) where pre_in is given -> dict(y, acc)"""
    acc = x.double() @ _d(wt, x).t() + _d(bias, x)
    return dict(y=r(acc if pre_in is None else acc * nr.gelu_grad64(pre_in.double())), acc=acc)


def mlp_fwd(a, res, k, w1f, b1f, w2, b2, r, eps=EPS):
    """clv_mlp_fused_fwd -> dict(out, s, mean, rstd, xhat, h, act); ts = s, or a when there is no residual"""
    t = _stream(a, res, k)
    mu, rstd = _stats(t, eps)
    xhat = r((t - mu) * rstd)
    h = xhat @ _d(w1f, a).t() + _d(b1f, a)
    act = r(nr.gelu64(h))
    out = r(act @ _d(w2, a).t() + _d(b2, a))
    return dict(out=out, s=r(t), mean=mu.squeeze(-1), rstd=rstd.squeeze(-1), xhat=xhat, h=h, act=act)


def mlp_bwd(ts, mean, rstd, dout, dsum, k, w1f, b1f, w2, r, want_dres=True):
    """clv_mlp_fused_bwd from the STORED stream ts and the forward's statistics -> dict(da, dres, xhat, act, dpre, h, dact)"""
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xhat = r((ts.double() - mu) * rs)
    h = xhat @ _d(w1f, ts).t() + _d(b1f, ts)
    act = r(nr.gelu64(h))
    dact = dout.double() @ _d(w2, ts)
    dpre = r(dact * nr.gelu_grad64(h))
    g = dpre @ _d(w1f, ts)
    dt = rs * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    if dsum is not None:
        dt = dt + dsum.double()
    da = r(dt if k is None else dt * _d(k, ts)[:, None])
    return dict(da=da, dres=r(dt) if want_dres else None, xhat=xhat, act=act, dpre=dpre, h=h, dact=dact)


def by_rows(fn, rows, others, chunk=16384):
    """fn(*row tensors, *others) -> dict of per-row tensors, evaluated in row chunks and concatenated (None rows / outputs stay
    None): keeps the fp64 temporaries of the large cases small."""
    M = next(t for t in rows if t is not None).shape[0]
    parts = [fn(*[None if t is None else t[i:i + chunk] for t in rows], *others) for i in range(0, M, chunk)]
    return {key: None if parts[0][key] is None else torch.cat([p[key] for p in parts]) for key in parts[0]}


# ----------------------------------------------------------------------------------------------- allowances
def erf_gelu_allow(pre):
    return nr.spacing16(nr.gelu64(pre), HALF) + gr.GELU_TERM * pre.abs()


def erf_gelu_grad_allow(pre):
    return nr.spacing16(nr.gelu_grad64(pre), HALF) + gr.GELU_GRAD_TERM * (1 + pre.abs())


def fast_gelu_allow(x):
    return nr.spacing16(nr.gelu64(x), HALF) + FAST_GELU_ABS + gr.GELU_TERM * x.abs()


def fast_gelu_grad_allow(x):
    return nr.spacing16(nr.gelu_grad64(x), HALF) + FAST_GELU_GRAD_ABS + gr.GELU_GRAD_TERM * (1 + x.abs())


# ----------------------------------------------------------------------------------------------- generators
def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 17) % (1 << 62)
    return torch.Generator().manual_seed(seed)


def pm1_rows(M, K, g):
    """[M][K] fp32: every row a random permutation of K/2 values +1 and K/2 values -1"""
    rank = torch.rand(M, K, generator=g).argsort(1).argsort(1)
    return torch.where(rank < K // 2, 1.0, -1.0)


def split_stream(t, fac, rps, g):
    """(a, res) with a k + res == t exactly: samples of factor 1 get a in {0, +-2} and res = t - a, samples of factor 0
    res = t and an ARBITRARY a (Gaussian: it must not reach the stream).  fac [B] of 0 / 1."""
    M, K = t.shape
    k = fac.repeat_interleave(rps)[:M]
    assert set(fac.tolist()) <= {0.0, 1.0} and k.shape[0] == M
    a = torch.randint(-1, 2, (M, K), generator=g).float() * 2
    dead = (k == 0)[:, None]
    a = torch.where(dead, torch.randn(M, K, generator=g) * 3, a)
    res = torch.where(dead, t, t - a)
    return a, res, k


class StdCase(NamedTuple):
    a: torch.Tensor             # HALF [M][K]
    res: Optional[torch.Tensor]
    fac: Optional[torch.Tensor]  # fp32 [B] or None
    rps: int
    k: Optional[torch.Tensor]   # fp32 [M] the factor of every row, or None
    t: torch.Tensor             # fp32 [M][K]: the +-1 pattern = s = xhat
    wt: torch.Tensor            # HALF [N][K]
    bias: torch.Tensor          # fp32 [N]
    acc: torch.Tensor           # fp64 [M][N] = t wt^T (on `device`)
    q: float


@functools.lru_cache(maxsize=None)
def std_exact_case(M, N, K, gelu, res=False, samples=0, device='cpu'):
    """The +-1 rows against ternary weights at the largest density that meets the caps of gemm_ref (gelu: weights in
    {0, +-1/8}, bias multiples of 1/16 in [-2, 2]; else {0, +-1} and integers in [-8, 8])."""
    q = 1 / 16 if gelu else 1.0
    why = None
    for i, dens in enumerate(gr.DENSITIES):
        g = _gen(M, N, K, gelu, res, samples, i)
        t = pm1_rows(M, K, g)
        wt = (gr._tern(g, dens, N, K) * (0.125 if gelu else 1.0)).to(HALF)
        bias = torch.randint(-32, 33, (N,), generator=g).float() / 16 if gelu else torch.randint(-8, 9, (N,), generator=g).float()
        a, r_, fac, rps, k = t, None, None, 1, None
        if res:
            B = samples or 1
            rps = M // B
            assert rps * B == M
            fac = factors(B, exact=True) if samples else torch.ones(1)
            a, r_, k = split_stream(t, fac, rps, g)
            if not samples:
                fac, k = None, None
        acc = gr.acc64(t.to(HALF), wt, device)
        try:
            gr.check_caps(t.to(HALF), wt, bias, acc, q)
        except AssertionError as e:
            why = e
            continue
        return StdCase(a.to(HALF), None if r_ is None else r_.to(HALF), fac, rps, k, t, wt, bias, acc, q)
    raise AssertionError(f'{M}x{N}x{K}: no density meets the caps ({why})')


class FmExact(NamedTuple):
    a: torch.Tensor
    res: Optional[torch.Tensor]
    fac: Optional[torch.Tensor]
    rps: int
    k: Optional[torch.Tensor]
    t: torch.Tensor             # fp32 [M][96], +-1
    w1f: torch.Tensor           # HALF [384][96] in {0, +-1/8}
    b1f: torch.Tensor           # fp32 [384], multiples of 1/16
    w2: torch.Tensor            # HALF [96][384] in {0, +-1}
    dout: torch.Tensor          # HALF [M][96] in {0, +-1}
    h: torch.Tensor             # fp64 [M][384]: the exact pre-activation
    dact: torch.Tensor          # fp64 [M][384]: the exact dout W2 (integers)


@functools.lru_cache(maxsize=None)
def fm_exact_case(M, variant, device='cpu'):
    why = None
    for i, dens in enumerate(gr.DENSITIES):
        g = _gen(M, FM_VARIANTS.index(variant), i, 4242)
        t = pm1_rows(M, FM_C, g)
        w1f = (gr._tern(g, dens, FM_H, FM_C) * 0.125).to(HALF)
        b1f = torch.randint(-32, 33, (FM_H,), generator=g).float() / 16
        w2 = gr._tern(g, dens, FM_C, FM_H).to(HALF)
        dout = gr._tern(g, dens, M, FM_C).to(HALF)
        a, r_, fac, rps, k = t, None, None, 1, None
        if variant != 'plain':
            B = samples_of(M) if variant == 'res_xscale' else 1
            rps = M // B
            fac = factors(B, exact=True) if variant == 'res_xscale' else torch.ones(1)
            a, r_, k = split_stream(t, fac, rps, g)
            if variant == 'res':
                fac, k = None, None
        h_acc = gr.acc64(t.to(HALF), w1f, device)
        dact = gr.acc64(dout, w2.t().contiguous(), device)
        try:
            gr.check_caps(t.to(HALF), w1f, b1f, h_acc, 1 / 16)
            gr.check_caps(dout, w2.t().contiguous(), torch.zeros(FM_H), dact, 1.0)
        except AssertionError as e:
            why = e
            continue
        return FmExact(a.to(HALF), None if r_ is None else r_.to(HALF), fac, rps, k, t, w1f, b1f, w2, dout,
                       h_acc + b1f.double().to(device), dact)
    raise AssertionError(f'one-kernel MLP, M = {M}: no density meets the caps ({why})')


def gauss(seed, *shape, scale=1.0, device='cpu'):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=device) * scale


def gelu_sweep_points():
    """fp32 points of the pointwise fast-GELU sweep, padded with zeros to a multiple of 384"""
    nf = lambda v, d: torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(d, dtype=torch.float32)).item()   # noqa: E731
    pts = [torch.linspace(-6, 6, 12288, dtype=torch.float64).float()]
    edge = [s * v for s in (1.0, -1.0) for v in (5.5, nf(5.5, 10.0), nf(5.5, 0.0))]
    tiny = [0.0, -0.0] + [s * 2.0 ** -k_ for s in (1.0, -1.0) for k_ in range(1, 25)]
    far = [s * (6 + 0.25 * i) for s in (1.0, -1.0) for i in range(41)]
    pts.append(torch.tensor(edge + tiny + far, dtype=torch.float32))
    p = torch.cat(pts)
    pad = (-p.numel()) % FM_H
    return torch.cat([p, torch.zeros(pad)]).view(-1, FM_H)
