"""References for the optimizer kernels (clover_amd/csrc/optim.hip), on the CPU: the fp64 sum of squares, the AdamW update
of ``adam_one`` in fp64 and as an fp32 floor, a plain-Python model of ``optim_prep_kernel`` with its loss scaler, and the
input builders of tests/test_optim_gpu.py.  Each builder's conditions are asserted in tests/test_optim_ref_cpu.py; the
bounds and their reasoning are in tests/OPTIM_ERROR_BUDGET.md."""
import ctypes as C
import math

import numpy as np
import torch

U32 = 2.0 ** -24                       # unit roundoff of fp32
CAP = 2 ** 24                          # integers below it are exact in fp32, and so is every partial sum of such data
FLT_MAX = float(np.finfo(np.float32).max)
SUMSQ, ADAMW, PACK = 0, 1, 2           # `kind` of clv_optim_plan
SUMSQ_CHUNK, SUMSQ_SLOTS, SLOT_STRIDE = 16384, 64, 16
GUARD = 1024                           # NaN sentinel elements on either side of every output

# Roundings that feed one output of adam_one, first order, each counted against the sum of term magnitudes the reference
# returns (OPTIM_ERROR_BUDGET.md, Bounds).  m': (1 - b1), g coef, their product, b1 m, the sum.  v': (1 - b2), g coef twice,
# two products, b2 v, the sum.  p': see p_cap().
R_M, R_V, R_P = 4, 6, 14


def f32(x):
    return float(np.float32(x))


def _np64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().double().numpy()
    return np.asarray(a, dtype=np.float64)


def sumsq64(g):
    """The fp64 sum of squares of g (a tensor or an array of any float type)."""
    a = _np64(g).reshape(-1)
    return float(np.dot(a, a))


def adamw64(p, g, m, v, coef, bc1, bc2_sqrt, lr, beta1, beta2, eps, wd):
    """adam_one in fp64 on the fp32 values the kernel receives (the hyper-parameters cross the C ABI as floats).
    -> p', m', v', (|p decay| + |step|, |b1 m| + |(1 - b1) g coef|, v'): the term-magnitude sums errors are divided by."""
    p, g, m, v = (_np64(a) for a in (p, g, m, v))
    lr, beta1, beta2, eps, wd = (f32(a) for a in (lr, beta1, beta2, eps, wd))     # coef, bc1, bc2_sqrt: as given
    g = g * coef
    pd = p * (1.0 - lr * wd)
    t1, t2 = beta1 * m, (1.0 - beta1) * g
    m1 = t1 + t2
    v1 = beta2 * v + (1.0 - beta2) * g * g
    denom = np.sqrt(v1) / bc2_sqrt + eps
    step = (lr / bc1) * (m1 / denom)
    return pd - step, m1, v1, (np.abs(pd) + np.abs(step), np.abs(t1) + np.abs(t2), v1)


def adamw_floor32(p, g, m, v, coef, bc1, bc2_sqrt, lr, beta1, beta2, eps, wd):
    """The floor: the same formulas in numpy float32, one rounding per operation, in the order adam_one writes them and
    uncontracted (no fused multiply-add).  -> p', m', v' (float32 arrays)."""
    F = np.float32
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    coef, bc1, bc2_sqrt, lr, beta1, beta2, eps, wd = (F(a) for a in (coef, bc1, bc2_sqrt, lr, beta1, beta2, eps, wd))
    one = F(1)
    g = g * coef
    p = p * (one - lr * wd)
    m = beta1 * m + (one - beta1) * g
    v = beta2 * v + ((one - beta2) * g) * g
    denom = np.sqrt(v) / bc2_sqrt + eps
    p = p - (lr / bc1) * (m / denom)
    assert p.dtype == m.dtype == v.dtype == F
    return p, m, v


def cancellation(sums_m, m1):
    """kappa = (|b1 m| + |(1 - b1) g coef|) / |m'| per element (1 where m' = 0: then both terms are 0 or the step is 0)."""
    m1 = np.abs(m1)
    return np.where(m1 > 0, sums_m / np.where(m1 > 0, m1, 1.0), 1.0)


def p_cap(kappa):
    """Per-element cap on |p'_kernel - p'_64| / (|p decay| + |step|), in units of 2^-24.  step = (lr / bc1) (m' / denom):
    lr / bc1 1, the division 1, the product 1, denom 6 (v' 6, halved by the square root: 3; sqrtf 1, / bc2_sqrt 1, + eps 1),
    m' R_M kappa (a cancellation in m' is carried into the step undiminished); p decay: 3 (lr wd, 1 - , the product), the
    smaller branch; the final subtraction 1.  kappa = 1 gives R_P."""
    return 3 + 6 + R_M * kappa + 1


def rel_err(got, ref, sums):
    """|got - ref| / sums per element, 0 where the sum of term magnitudes is 0 (then got must be 0 as well)."""
    got, ref = _np64(got), _np64(ref)
    d = np.abs(got - ref)
    assert (d[sums == 0] == 0).all()
    return np.where(sums > 0, d / np.where(sums > 0, sums, 1.0), 0.0)


# ------------------------------------------------------------------------------------------------------------ optim_prep
STATE_FIELDS = ('coef', 'bc1', 'bc2_sqrt', 'norm', 'skip', 't', 'skipped', 'grad_loss_scale', 'loss_scale', 'scale_factor',
                'scale_window', 'scale_iter', 'last_overflow', 'dynamic')
STATE_FLOATS = ('coef', 'bc1', 'bc2_sqrt', 'norm', 'grad_loss_scale', 'loss_scale', 'scale_factor')
BIG = f32(3.0e38)                      # the kernel's overflow threshold, as the float it compares with


def new_state(**kw):
    st = dict.fromkeys(STATE_FIELDS, 0)
    st.update(coef=0.0, bc1=0.0, bc2_sqrt=0.0, norm=0.0, grad_loss_scale=0.0, loss_scale=0.0, scale_factor=0.0, last_overflow=0)
    st.update(kw)
    return st


def prep_ref(state, raw, beta1, beta2, max_norm, grad_scale):
    """optim_prep_kernel on the record `state` (a dict of STATE_FIELDS) and the raw sum of squares it reads; float fields
    in fp64 from the fp32 arguments.  -> the new record.  raw may be inf or NaN."""
    o = dict(state)
    beta1, beta2, max_norm, gs, raw = f32(beta1), f32(beta2), f32(max_norm), f32(grad_scale), float(raw)
    o['grad_loss_scale'] = o['loss_scale']                       # what this step's gradients carry, before the scale moves
    if o['loss_scale'] > 0:
        gs = gs / o['loss_scale']
    ss = raw * gs * gs
    if ss > FLT_MAX:
        ss = math.inf                                            # the kernel's product is an fp32 one
    overflow = math.isnan(ss) or ss > BIG or raw > BIG
    if overflow:
        o['skip'] = 1
        o['skipped'] += 1
        o['norm'] = ss
    else:
        o['skip'] = 0
        o['t'] += 1
        o['norm'] = math.sqrt(ss)
        c = gs
        if max_norm > 0:
            c *= min(max_norm / (o['norm'] + f32(1e-6)), 1.0)
        o['coef'] = c
        o['bc1'] = 1.0 - beta1 ** o['t']
        o['bc2_sqrt'] = math.sqrt(1.0 - beta2 ** o['t'])
    if o['dynamic'] and o['loss_scale'] > 0:                     # LossScaler.update_scale
        if overflow:
            o['loss_scale'] = max(o['loss_scale'] / o['scale_factor'], 1.0)
            o['last_overflow'] = o['scale_iter']
        elif o['scale_window'] > 0 and (o['scale_iter'] - o['last_overflow']) % o['scale_window'] == 0:
            o['loss_scale'] = o['loss_scale'] * o['scale_factor']
        o['scale_iter'] += 1
    return o


def overflow_pattern(steps=40):
    """The overflow steps of the scaler trajectory: runs of overflows long enough to drive a scale of 2 to the floor,
    windows between them long enough for the scale to grow again (window 3), fixed."""
    hit = {2, 3, 4, 5, 11, 19, 20, 30, 31, 32, 33}
    return [i in hit for i in range(steps)]


def ulps32(got, ref):
    """|got - ref| in units of the fp32 spacing at ref (ref an fp64 value; both inf, or both NaN: 0)."""
    if math.isnan(ref) or math.isnan(got):
        return 0.0 if math.isnan(ref) and math.isnan(got) else math.inf
    if math.isinf(ref) or math.isinf(got):
        return 0.0 if ref == got else math.inf
    if ref == got:
        return 0.0
    return abs(got - ref) / float(np.spacing(np.float32(abs(ref))))


# -------------------------------------------------------------------------------------------------------- input builders
def int_grad(n, seed):
    """n integers in [-2, 2] with a few +-8 (all exact in either 16-bit type), float32; the total sum of squares plus the
    5.0 the accumulator starts at stays below 2^24, so every fp32 summation order gives the same, exact, result."""
    rng = np.random.default_rng(seed)
    g = rng.integers(-2, 3, size=n).astype(np.float32)
    k = min(n, 8)
    g[rng.choice(n, size=k, replace=False)] = rng.choice(np.array([-8.0, 8.0], dtype=np.float32), size=k)
    assert 5 + sumsq64(g) < CAP
    return g


def needle(n, pos):
    g = np.zeros(n, dtype=np.float32)
    g[pos] = 3.0
    return g


EPS = 1e-8
COEFS = (1.0, 0.37, 2.0 ** -16)        # the clip coefficients the AdamW cases run under
KAPPA_MAX = 3.0                        # wide_state: |b1 m| and |(1 - b1) g coef| of opposite sign differ by a factor >= 2


def wide_state(n, seed, bc2_sqrt):
    """p, g, m, v (float32) that reach every branch of adam_one's arithmetic: p ~ 0.05 N(0,1) with exact zeros; |g|
    log-uniform in [1e-9, 1e2] with random sign and exact zeros; m of either sign relative to g; v >= 0 with exact zeros
    (g = m = v = 0 together among them) and values at which sqrt(v) / bc2_sqrt is far below, around and far above eps.
    Everything is zero or a normal fp32 number of magnitude >= 1e-30.  Where m and g oppose each other, m is moved (by
    factors of 4) until the two terms of m' differ by a factor of at least 2 under every coefficient of COEFS (beta1 = 0.9):
    the cancellation kappa stays <= KAPPA_MAX, so that no handful of elements whose m' nearly vanishes decides the
    statistics of p' (p_cap() says how a cancellation enters p')."""
    rng = np.random.default_rng(seed)
    p = 0.05 * rng.standard_normal(n)
    g = 10.0 ** rng.uniform(-9, 2, n) * rng.choice([-1.0, 1.0], n)
    m = 10.0 ** rng.uniform(-9, 2, n) * rng.choice([-1.0, 1.0], n)
    v = 10.0 ** rng.uniform(-24, 2, n)
    k = np.arange(n)
    mid = (EPS * f32(bc2_sqrt)) ** 2                         # sqrt(v) / bc2_sqrt == eps
    v[k % 16 == 3] = mid * 10.0 ** rng.uniform(-0.3, 0.3, n)[k % 16 == 3]
    p[k % 16 == 5] = 0
    g[k % 16 == 7] = 0
    v[k % 16 == 9] = 0
    g[k % 16 == 11] = 0; m[k % 16 == 11] = 0; v[k % 16 == 11] = 0
    v[k % 32 == 13] = 0; g[k % 32 == 13] = 0                # v' = 0 with m != 0: the step is m' / eps
    g, m = g.astype(np.float32).astype(np.float64), m.astype(np.float32)
    for _ in range(64):
        mm = m.astype(np.float64)
        bad = np.zeros(n, dtype=bool)
        for c in COEFS:
            a, b = np.abs(f32(0.9) * mm), np.abs((1 - f32(0.9)) * g * f32(c))
            bad |= (mm * g < 0) & (a < 2.001 * b) & (b < 2.001 * a)
        if not bad.any():
            break
        m[bad] *= np.float32(4)
    assert not bad.any()
    out = [a.astype(np.float32) for a in (p, g, m, v)]
    for a in out:
        nz = np.abs(a[a != 0])
        assert nz.size == 0 or (nz.min() >= 1e-30 and np.isfinite(nz).all())
    return out


def half_layout(dtype):
    """(exponent bits, mantissa bits, bias) of the 16-bit type."""
    return (5, 10, 15) if dtype == torch.float16 else (8, 7, 127)


def half_magnitude(k, dtype):
    """The value of the non-negative 16-bit pattern k, in fp64; the first non-finite pattern decodes as the next power of
    two, so that the largest finite value has a midpoint above it as well."""
    E, M, bias = half_layout(dtype)
    k = np.asarray(k, dtype=np.int64)
    e, f = k >> M, (k & ((1 << M) - 1)).astype(np.float64)
    return np.where(e == 0, np.ldexp(f, 1 - bias - M), np.ldexp(f + (1 << M), (e - bias - M).astype(np.int64)))


def pack_table(dtype):
    """fp32 inputs of the pack kernel: for every finite value h of the 16-bit type and either sign, h itself, the midpoint
    between h and its successor in magnitude (a tie), and that midpoint one fp32 ulp down and up; then +-inf, NaN, the
    largest finite fp32 and values that overflow the 16-bit type.  -> (float32 tensor, number of finite patterns K)."""
    E, M, _ = half_layout(dtype)
    K = ((1 << E) - 1) << M                                  # patterns 0 .. K-1 are finite and non-negative
    k = np.arange(K)
    h, nxt = half_magnitude(k, dtype), half_magnitude(k + 1, dtype)
    mid = ((h + nxt) / 2).astype(np.float32)
    assert (mid.astype(np.float64) == (h + nxt) / 2).all() and np.isfinite(mid).all()      # every midpoint is an fp32 number
    below, above = np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))
    mag = np.stack([h.astype(np.float32), mid, below, above], 1).reshape(-1)
    special = np.array([np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX, 7.0e4, -7.0e4, 3.4e38, -3.4e38, 1.0e30], dtype=np.float32)
    return torch.from_numpy(np.concatenate([mag, -mag, special])), K


def count_ties(x, dtype):
    """Elements of the fp32 tensor x that lie exactly halfway between two neighbouring values of the 16-bit type, decided
    from the type's spacing alone (no conversion involved)."""
    E, M, bias = half_layout(dtype)
    a = np.abs(x.double().numpy())
    a = a[np.isfinite(a) & (a > 0)]
    ex = np.maximum(np.frexp(a)[1] - 1, 1 - bias)            # floor(log2 a), held at the smallest normal exponent
    y = np.ldexp(a, -(ex - M - 1))                           # a in units of half the spacing
    return int(((y == np.floor(y)) & (np.floor(y) % 2 == 1)).sum())


# ------------------------------------------------------------------------------------------------------- launch classes
TAIL_ONLY, ONE_BLOCK, MANY_BLOCKS, TWO_TRIPS = 'tail only', 'one block', 'many blocks, one trip', 'two trips for some threads'
SUMSQ_SIZES = {1: TAIL_ONLY, 2: TAIL_ONLY, 3: TAIL_ONLY, 4: ONE_BLOCK, 1024: ONE_BLOCK, 1027: ONE_BLOCK,
               262145: MANY_BLOCKS, 262146: MANY_BLOCKS, 262147: MANY_BLOCKS, 2098355: TWO_TRIPS}
TWO_TRIP_N = 2098355                                         # 4 (2048 256 + 300) + 3
TRIP2_FIRST = 4 * 2048 * 256                                 # element 2 097 152: the first one of the second trip
ADAMW_SIZES = {1: TAIL_ONLY, 2: TAIL_ONLY, 3: TAIL_ONLY, 4: ONE_BLOCK, 5: ONE_BLOCK, 7: ONE_BLOCK, 1023: ONE_BLOCK,
               1024: ONE_BLOCK, 1025: ONE_BLOCK, 1027: ONE_BLOCK, 262147: MANY_BLOCKS}
PACK_SIZES = {1: TAIL_ONLY, 2: TAIL_ONLY, 3: TAIL_ONLY, 4: ONE_BLOCK, 5: ONE_BLOCK, 1027: MANY_BLOCKS}
RANGE_LENGTHS = (1, 3, 4, 7, 16383, 16384, 16385, 40001)


def plan(lib, kind, n):
    from clover_amd import _lib
    out = _lib.ClvOptimPlan()
    rc = lib.clv_optim_plan(kind, n, C.byref(out))
    assert rc == 0, (kind, n, rc)
    return out


def launch_class(pl, n):
    """The class of a launch from its plan record."""
    assert pl.block == 256 and pl.tail == n % 4
    if pl.trips == 0:
        assert pl.grid == 1 and n < 4
        return TAIL_ONLY
    if pl.trips == 1:
        return ONE_BLOCK if pl.grid == 1 else MANY_BLOCKS
    assert pl.trips == 2 and n // 4 < 2 * pl.grid * pl.block                       # the last threads make one trip only
    return TWO_TRIPS


def sumsq_depth(pl):
    """The longest chain of fp32 additions a term of clv_sumsq passes through: 4 per trip of its thread (three inside the
    float4's sum, one into the running sum), 6 across the wave, 3 across the block's four waves, and at most gridDim
    atomic additions."""
    return 4 * pl.trips + 6 + 3 + pl.grid
