"""Every launch class of the optimizer kernels (csrc/optim.hip: the gradient norm, the device-side step decision with its
loss scaler, AdamW with the 16-bit shadow, the wire copy) through the C entries, and once per entry through
clover_amd.ops.  Integer data and bit patterns are compared exactly; everything else against the fp64 references of
tests/optim_ref.py, under bounds that come from counted roundings and from the fp32 floor of the same module (2 x its RMS,
4 x its maximum) — never from the kernels.  Every output sits between NaN guards on its own allocation.
tests/OPTIM_ERROR_BUDGET.md has the classes, the reasoning and the measured table.  `-m gpu` only."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
G = R.GUARD
RMS_X, MAX_X = 2.0, 4.0                         # margins over the floor (test_attention_gpu.py, test_norm_act_gpu.py)
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.98, R.EPS, 0.05
STAT_MIN_N = 1023                               # a tensor of fewer elements has no RMS of its own: see floor_stats()
NWIDE = 262147


def L():
    from clover_amd import _lib
    return _lib.lib()


def HALF():
    from clover_amd import _lib
    return _lib.half_dtype()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, byte_offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + byte_offset)


class Guarded:
    """A tensor of n elements at an aligned offset of a larger allocation, NaN on either side (and inside, unless values
    are given); `extra` more elements behind it belong to the view's allocation but not to the operand (a shadow's pad)."""

    def __init__(self, n, dtype=torch.float32, values=None, extra=0, lead=0):
        self.n, self.lo = n, G + lead
        self.buf = torch.full((G + lead + n + extra + G,), float('nan'), dtype=dtype, device=DEV)
        self.t = self.buf[self.lo:self.lo + n]
        assert lead or self.t.data_ptr() % 16 == 0
        if values is not None:
            self.t.copy_(torch.as_tensor(values).to(dtype))

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all() and torch.isnan(self.buf[self.lo + self.n:]).all())

    def bits(self):
        return self.buf.view(torch.int32 if self.buf.element_size() == 4 else torch.int16).cpu().clone()

    def np(self):
        return self.t.float().cpu().numpy() if self.t.dtype != torch.float32 else self.t.cpu().numpy()


def hbits(t):
    return t.contiguous().view(torch.int16).cpu()


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

    def done(self):
        print('OPTIMBUDGET', self.name, ' '.join(f'{k}={g:.3e}/{a:.3e}({r:.2f})' for k, (r, g, a) in sorted(self.worst.items())))
        assert not self.bad, self.bad[:8]


# ==================================================================================================== clv_sumsq(_bf16)
def sumsq_call(vals, is16, acc0=5.0):
    """One launch of clv_sumsq / clv_sumsq_bf16 on a guarded view of vals (NaN all around: an over-read poisons the sum).
    -> acc[0]."""
    n = len(vals)
    g = Guarded(n, HALF() if is16 else torch.float32, values=torch.from_numpy(np.asarray(vals)))
    acc = Guarded(1, values=[acc0])
    fn = L().clv_sumsq_bf16 if is16 else L().clv_sumsq
    assert fn(ptr(g.t), ptr(acc.t), n, stream()) == 0
    torch.cuda.synchronize()
    assert acc.guards_intact()
    return acc.t.item(), g


@pytest.mark.parametrize('is16', [0, 1], ids=['fp32', '16bit'])
@pytest.mark.parametrize('n', sorted(R.SUMSQ_SIZES))
def test_sumsq_integer_data_is_exact(n, is16):
    assert R.launch_class(R.plan(L(), R.SUMSQ, n), n) == R.SUMSQ_SIZES[n]
    g = R.int_grad(n, n)
    got, _ = sumsq_call(g, is16)
    assert got == 5.0 + R.sumsq64(g)
    spots = {0, max(0, (n // 4 - 1) * 4)} | {n - 1 - i for i in range(n % 4)}                 # first, last float4, each tail place
    if n == R.TWO_TRIP_N:
        spots |= {R.TRIP2_FIRST, R.TRIP2_FIRST - 1}
    for pos in sorted(spots):
        got, _ = sumsq_call(R.needle(n, pos), is16, acc0=0.0)
        assert got == 9.0, pos


@functools.lru_cache(maxsize=None)
def normal(n):
    return torch.randn(n, generator=torch.Generator().manual_seed(n), dtype=torch.float32)


@pytest.mark.parametrize('is16', [0, 1], ids=['fp32', '16bit'])
@pytest.mark.parametrize('n', sorted(R.SUMSQ_SIZES))
def test_sumsq_random_data_within_the_depth_bound(n, is16):
    pl = R.plan(L(), R.SUMSQ, n)
    bud = Budget(f'sumsq n={n} {"16bit" if is16 else "fp32"} grid={pl.grid} trips={pl.trips}')
    for s in (1e-3, 1.0, 300.0):
        x = normal(n) * s
        if is16:
            x = x.to(HALF()).float()                                   # the reference sums what the kernel reads
        ref = R.sumsq64(x)
        got, _ = sumsq_call(x.numpy(), is16, acc0=0.0)
        bud.check('rel', abs(got - ref) / ref if ref else abs(got), R.sumsq_depth(pl) * R.U32, s)
    bud.done()


def test_sumsq_of_nothing_and_refusals():
    lib = L()
    acc = Guarded(1, values=[5.0])
    g = Guarded(8, values=np.ones(8, np.float32))
    before = acc.bits()
    assert lib.clv_sumsq(ptr(g.t), ptr(acc.t), 0, stream()) == 0 and lib.clv_sumsq_bf16(ptr(g.t), ptr(acc.t), 0, stream()) == 0
    assert lib.clv_sumsq(ptr(g.t, 4), ptr(acc.t), 4, stream()) == -1             # off by one float
    assert lib.clv_sumsq_bf16(ptr(g.t, 4), ptr(acc.t), 4, stream()) == -1        # off by two 16-bit elements
    assert lib.clv_sumsq(ptr(g.t), ptr(acc.t), -1, stream()) == -1 and lib.clv_sumsq(None, ptr(acc.t), 4, stream()) == -1
    assert lib.clv_sumsq(ptr(g.t), None, 4, stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(acc.bits(), before)


# ==================================================================================================== clv_sumsq_ranges
def range_layout():
    """The ranges of RANGE_LENGTHS in one buffer, 4-aligned starts with NaN gaps between them, cut into table rows of at
    most SUMSQ_CHUNK floats, with one row of count 0 in the middle.  -> (values, rows)."""
    vals, rows, a = [], [], 12
    for i, n in enumerate(R.RANGE_LENGTHS):
        vals.append((a, R.int_grad(n, 700 + i)))
        b = a
        while b < a + n:
            c = min(R.SUMSQ_CHUNK, a + n - b)
            rows.append((b, c))
            b += c
        if i == 3:
            rows.append((a, 0))                                         # written by hand: must add nothing
        a = (a + n + 3) // 4 * 4 + 8
    return vals, rows, a


def test_sumsq_ranges_reads_its_ranges_and_nothing_else():
    from clover_amd import ops
    lib = L()
    vals, rows, total = range_layout()
    base = Guarded(total)
    want = 5.0
    for a, g in vals:
        base.t[a:a + len(g)] = torch.from_numpy(g).to(DEV)
        want += R.sumsq64(g)
    assert want < R.CAP and len(rows) == 1 + sum(-(-n // R.SUMSQ_CHUNK) for n in R.RANGE_LENGTHS)
    assert all(a % 4 == 0 and 0 <= c <= R.SUMSQ_CHUNK for a, c in rows) and torch.isnan(base.t).sum() > 8 * len(vals)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    acc = Guarded(4)
    acc.t[0] = 5.0
    assert lib.clv_sumsq_ranges(ptr(base.t), ptr(table), len(rows), ptr(acc.t), stream()) == 0
    torch.cuda.synchronize()
    assert acc.t[0].item() == want and torch.isnan(acc.t[1:]).all() and acc.guards_intact()
    before = acc.bits()
    assert lib.clv_sumsq_ranges(ptr(base.t), ptr(table), 0, ptr(acc.t), stream()) == 0             # no rows: no launch
    assert lib.clv_sumsq_ranges(ptr(base.t, 4), ptr(table), len(rows), ptr(acc.t), stream()) == -1
    assert lib.clv_sumsq_ranges(ptr(base.t), ptr(table, 4), len(rows), ptr(acc.t), stream()) == -1
    assert lib.clv_sumsq_ranges(ptr(base.t), ptr(table), -1, ptr(acc.t), stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(acc.bits(), before)
    # the same ranges through ops (its own table, without the empty row)
    t2, nb = ops.sumsq_range_table([(a, a + len(g)) for a, g in vals], DEV)
    assert nb == len(rows) - 1
    ops.sumsq_ranges(base.t, t2, nb, acc.t)
    assert acc.t[0].item() == 2 * want - 5.0


# ======================================================================================================= clv_pack_bf16
@functools.lru_cache(maxsize=None)
def pack_inputs():
    x, K = R.pack_table(HALF())
    return x, x.to(HALF()), K


def pack_check(x, want, fn):
    n = x.numel()
    src = Guarded(n, values=x)
    dst = Guarded(n, HALF())
    fn(src.t, dst.t)
    torch.cuda.synchronize()
    got = dst.t.cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    bad = (hbits(got) != hbits(want)) & ~nan
    assert not bad.any(), [(float(a), hex(int(b) & 0xffff), hex(int(c) & 0xffff)) for a, b, c in
                           zip(x[bad][:8], hbits(got)[bad][:8], hbits(want)[bad][:8])]
    assert dst.guards_intact()


def c_pack(src, dst):
    assert L().clv_pack_bf16(ptr(src), ptr(dst), src.numel(), stream()) == 0


def test_pack_rounds_every_value_and_every_tie_to_nearest_even():
    x, want, K = pack_inputs()
    assert R.launch_class(R.plan(L(), R.PACK, x.numel()), x.numel()) == R.MANY_BLOCKS
    pack_check(x, want, c_pack)


@pytest.mark.parametrize('n', sorted(R.PACK_SIZES))
def test_pack_sizes(n):
    from clover_amd import ops
    assert R.launch_class(R.plan(L(), R.PACK, n), n) == R.PACK_SIZES[n]
    x, want, K = pack_inputs()
    a = 4 * 15361                                                       # a stretch of the table with ties in it
    pack_check(x[a:a + n].clone(), want[a:a + n].clone(), c_pack)
    if n == 1027:
        pack_check(x[a:a + n].clone(), want[a:a + n].clone(), ops.pack_bf16)


def test_pack_of_nothing_and_refusals():
    lib = L()
    src, dst = Guarded(8, values=np.ones(8, np.float32)), Guarded(8, HALF())
    before = dst.bits()
    assert lib.clv_pack_bf16(ptr(src.t), ptr(dst.t), 0, stream()) == 0
    assert lib.clv_pack_bf16(ptr(src.t, 4), ptr(dst.t), 4, stream()) == -1
    assert lib.clv_pack_bf16(ptr(src.t), ptr(dst.t, 2), 4, stream()) == -1
    assert lib.clv_pack_bf16(ptr(src.t), ptr(dst.t), -1, stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(dst.bits(), before)


# ================================================================================== clv_optim_prep / clv_optim_prep_slots
INT_AT = dict(skip=4, t=5, skipped=6, scale_window=10, scale_iter=11, last_overflow=12, dynamic=13)
FLOAT_AT = dict(coef=0, bc1=1, bc2_sqrt=2, norm=3, grad_loss_scale=7, loss_scale=8, scale_factor=9)


def state_write(st):
    """The 64-byte record with every field of the dict st, as a device int32 tensor (the test's own writer)."""
    raw = np.zeros(16, dtype=np.int32)
    f = raw.view(np.float32)
    for k, i in INT_AT.items():
        raw[i] = st[k]
    for k, i in FLOAT_AT.items():
        f[i] = st[k]
    return torch.from_numpy(raw).to(DEV)


def state_read(t):
    raw = t.cpu().numpy()
    f = raw.view(np.float32)
    st = {k: int(raw[i]) for k, i in INT_AT.items()}
    st.update({k: float(f[i]) for k, i in FLOAT_AT.items()})
    assert raw[14] == 0 and raw[15] == 0
    return st


def prep_call(st, raw, max_norm, grad_scale, slots=None, b1=B1, b2=B2):
    state = state_write(st)
    acc = Guarded(1, values=[raw])
    fn = L().clv_optim_prep
    if slots is None:
        rc = fn(ptr(acc.t), ptr(state), b1, b2, max_norm, grad_scale, stream())
    else:
        rc = L().clv_optim_prep_slots(ptr(acc.t), ptr(slots), ptr(state), b1, b2, max_norm, grad_scale, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert acc.t.item() == 0.0 and acc.guards_intact()                 # re-zeroed for the next step
    return state_read(state)


def prep_compare(got, want, before, bud, where):
    for k in INT_AT:
        assert got[k] == want[k], (where, k, got[k], want[k])
    for k in ('loss_scale', 'scale_factor', 'grad_loss_scale'):
        assert got[k] == want[k], (where, k, got[k], want[k])
    if want['skip']:
        for k in ('coef', 'bc1', 'bc2_sqrt'):
            assert got[k] == before[k], (where, k)                       # a skipped step leaves them alone
        bud.check('norm.ulp', R.ulps32(got['norm'], want['norm']), 2.0, where)
    else:
        bud.check('norm.ulp', R.ulps32(got['norm'], want['norm']), 2.0, where)
        bud.check('coef.ulp', R.ulps32(got['coef'], want['coef']), 2.0, where)
        bud.check('bc1.ulp', R.ulps32(got['bc1'], want['bc1']), 1.0, where)
        bud.check('bc2.ulp', R.ulps32(got['bc2_sqrt'], want['bc2_sqrt']), 1.0, where)


PRESET = dict(coef=0.25, bc1=0.5, bc2_sqrt=0.75, norm=-1.0, t=3, skipped=2)
PREP_CASES = [
    # name, state, raw, max_norm, grad_scale
    ('clip inactive', {}, 2.0, 10.0, 1.0),
    ('clip active', {}, 9.0 * 2 ** 20, 1.0, 1.0),
    ('norm == max_norm', {}, 16.0, 4.0, 1.0),
    ('max_norm 0, grad_scale 1/3', {}, 144.0, 0.0, 1.0 / 3.0),
    ('raw inf', {}, math.inf, 1.0, 1.0),
    ('raw nan', {}, math.nan, 1.0, 1.0),
    ('raw 3.2e38, scaled sum finite', {}, R.f32(3.2e38), 1.0, 2.0 ** -20),
    ('raw 1e30, scaled sum overflows', {}, R.f32(1e30), 1.0, 1e5),
    ('static scale 1024', dict(loss_scale=1024.0, scale_factor=2.0, scale_window=3, scale_iter=7, last_overflow=-1), 9.0 * 2 ** 20, 0.0, 1.0),
    ('static scale 1024, overflow', dict(loss_scale=1024.0, scale_factor=2.0, scale_window=3, scale_iter=7, last_overflow=-1), math.inf, 0.0, 1.0),
] + [(f't = {t}', dict(t=t), 2.0, 10.0, 1.0) for t in (0, 1, 9, 999, 99999)]


def test_prep_cases_against_the_model():
    bud = Budget('prep')
    for name, kw, raw, max_norm, gs in PREP_CASES:
        st = R.new_state(**{**PRESET, **kw})
        want = R.prep_ref(st, raw, B1, B2, max_norm, gs)
        got = prep_call(st, raw, max_norm, gs)
        prep_compare(got, want, st, bud, name)
        if 'max_norm 0' in name:
            assert got['coef'] == R.f32(gs)                              # bit for bit
        if 'static' in name:
            assert got['scale_iter'] == 7 and got['loss_scale'] == 1024.0
    assert R.prep_ref(R.new_state(), R.f32(3.2e38), B1, B2, 1.0, 2.0 ** -20)['skip'] == 1
    bud.done()


@pytest.mark.parametrize('init', [2.0 ** 20, 2.0])
def test_prep_dynamic_scaler_trajectory(init):
    bud = Budget(f'prep dynamic from {init}')
    st = R.new_state(loss_scale=init, scale_factor=2.0, scale_window=3, last_overflow=-1, dynamic=1)
    for i, over in enumerate(R.overflow_pattern()):
        raw = math.inf if over else st['loss_scale'] ** 2 * 4.0
        want = R.prep_ref(st, raw, B1, B2, 1.0, 1.0)
        got = prep_call(st, raw, 1.0, 1.0)
        assert got['grad_loss_scale'] == st['loss_scale']                # the scale BEFORE the move
        prep_compare(got, want, st, bud, i)
        st = got
    assert st['scale_iter'] == 40
    bud.done()


def test_prep_slots_adds_and_zeroes_the_slots_only():
    from clover_amd import ops
    for via_ops in (False, True):
        slots = Guarded(R.SUMSQ_SLOTS * R.SLOT_STRIDE)
        slots.t[::R.SLOT_STRIDE] = torch.arange(R.SUMSQ_SLOTS, dtype=torch.float32, device=DEV)
        total = sum(range(R.SUMSQ_SLOTS)) + 2080.0
        assert total == 4096.0
        st = R.new_state(**PRESET)
        if via_ops:
            state, acc = state_write(st), Guarded(1, values=[2080.0])
            ops.optim_prep(acc.t, state, B1, B2, 0.0, 1.0, slots=slots.t)
            torch.cuda.synchronize()
            got = state_read(state)
            assert acc.t.item() == 0.0 and acc.guards_intact()
        else:
            got = prep_call(st, 2080.0, 0.0, 1.0, slots=slots.t)
        assert got['norm'] == 64.0 and got['skip'] == 0 and got['t'] == 4 and got['coef'] == 1.0
        s = slots.t.cpu().view(R.SUMSQ_SLOTS, R.SLOT_STRIDE)
        assert (s[:, 0] == 0).all() and torch.isnan(s[:, 1:]).all() and slots.guards_intact()


def test_prep_refusals():
    lib = L()
    state, acc = state_write(R.new_state(**PRESET)), Guarded(1, values=[4.0])
    before = state.cpu().clone()
    assert lib.clv_optim_prep(ptr(acc.t), None, B1, B2, 1.0, 1.0, stream()) == -1
    assert lib.clv_optim_prep(ptr(acc.t), ptr(state, 2), B1, B2, 1.0, 1.0, stream()) == -1
    assert lib.clv_optim_prep(None, ptr(state), B1, B2, 1.0, 1.0, stream()) == -1
    assert lib.clv_optim_prep_slots(ptr(acc.t), None, None, B1, B2, 1.0, 1.0, stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(state.cpu(), before) and acc.t.item() == 4.0


# ========================================================================= clv_adamw_step_dev(_bf16g) / clv_adamw_step
def bias(t):
    """bias_c1, bias_c2 as the floats the host entry receives, and the bc2_sqrt its sqrtf makes of bias_c2."""
    bc1, bc2 = np.float32(1.0 - R.f32(B1) ** t), np.float32(1.0 - R.f32(B2) ** t)
    return float(bc1), float(bc2), float(np.sqrt(bc2))


@functools.lru_cache(maxsize=None)
def wide(t):
    return R.wide_state(NWIDE, 900 + t, bias(t)[2])


@functools.lru_cache(maxsize=None)
def wide_ref(coef, t, lr=LR, wd=WD, g16=False):
    """Reference, floor and their statistics for the whole wide state; a size n uses the first n elements of each."""
    p, g, m, v = wide(t)
    if g16:
        g = torch.from_numpy(g).to(HALF()).float().numpy()
    bc1, _, bc2s = bias(t)
    args = (coef, bc1, bc2s, lr, B1, B2, EPS, wd)
    p1, m1, v1, sums = R.adamw64(p, g, m, v, *args)
    fl = R.adamw_floor32(p, g, m, v, *args)
    ferr = [R.rel_err(a, b, s) for a, b, s in zip(fl, (p1, m1, v1), sums)]
    caps = [R.p_cap(R.cancellation(sums[1], m1)), np.full(NWIDE, float(R.R_M)), np.full(NWIDE, float(R.R_V))]
    for e, c in zip(ferr, caps):
        assert (e <= c * R.U32).all()                                    # the floor itself is inside the counted cap
    return (p1, m1, v1), sums, ferr, caps


def floor_stats(ferr, n):
    """RMS and maximum of the floor's error: over the same n elements when there are enough of them to have an RMS, over
    the whole population the elements are drawn from otherwise (one element's error is no estimate of either)."""
    e = ferr[:n] if n >= STAT_MIN_N else ferr
    return math.sqrt(float(np.mean(e * e))), float(e.max())


def adamw_call(entry, n, t, coef, shadow=True, lr=LR, wd=WD, skip=0, g16=False, inputs=None, sumsq=None, max_norm=0.0,
               shadow_fill=None, bc1=None, lead=None, n_arg=None, want_rc=0):
    """One launch of entry ('dev', 'dev16', 'host') on the first n elements of the wide state (or `inputs`), each operand
    between NaN guards.  `lead`: {operand: elements} moves that operand's view off its alignment.
    -> dict of the Guarded operands."""
    lib, lead = L(), lead or {}
    p, g, m, v = [a[:n] for a in (inputs or wide(t))]
    b1c, b2c, bc2s = bias(t)
    bc1 = b1c if bc1 is None else bc1
    pad = (-n) % 4
    o = dict(p=Guarded(n, values=p, lead=lead.get('p', 0)), m=Guarded(n, values=m, lead=lead.get('m', 0)),
             v=Guarded(n, values=v, lead=lead.get('v', 0)),
             g=Guarded(n, HALF() if entry == 'dev16' else torch.float32, values=g, lead=lead.get('g', 0)))
    o['sh'] = Guarded(n, HALF(), extra=pad, lead=lead.get('sh', 0)) if shadow else None
    if shadow and shadow_fill is not None:
        o['sh'].t.copy_(torch.as_tensor(shadow_fill[:n]).to(HALF()))
    sh = o['sh'].t if shadow else None
    n_arg = n if n_arg is None else n_arg
    before = {k: x.bits() for k, x in o.items() if x is not None}
    if entry == 'host':
        acc = None if sumsq is None else torch.tensor([sumsq], device=DEV)
        rc = lib.clv_adamw_step(ptr(o['p'].t), ptr(o['g'].t), ptr(o['m'].t), ptr(o['v'].t), ptr(sh), ptr(acc), n_arg, lr, B1,
                                B2, EPS, wd, bc1, b2c, max_norm, coef, stream())
    else:
        state = state_write(R.new_state(coef=coef, bc1=bc1, bc2_sqrt=bc2s, skip=skip, t=t))
        fn = lib.clv_adamw_step_dev_bf16g if entry == 'dev16' else lib.clv_adamw_step_dev
        rc = fn(ptr(o['p'].t), ptr(o['g'].t), ptr(o['m'].t), ptr(o['v'].t), ptr(sh), ptr(state), n_arg, lr, B1, B2, EPS, wd,
                stream())
    torch.cuda.synchronize()
    assert rc == want_rc, (entry, n, rc)
    for k, x in o.items():
        assert x is None or x.guards_intact(), (entry, n, k)             # the shadow's pad elements are guards too
    assert torch.equal(o['g'].bits(), before['g'])
    o['before'] = before
    return o


def unchanged(o, keys):
    return all(o[k] is None or torch.equal(o[k].bits(), o['before'][k]) for k in keys)


def same_bits(a, b, keys=('p', 'm', 'v', 'sh')):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k].bits(), b[k].bits()) for k in keys)


def shadow_is_rne_of_p(o):
    got = o['sh'].t.cpu()
    return torch.equal(hbits(got), hbits(o['p'].t.cpu().to(HALF())))


def adamw_budget(bud, o, n, ref, where):
    (p1, m1, v1), sums, ferr, caps = ref
    for k, want, s, fe, cap in zip(('p', 'm', 'v'), (p1, m1, v1), sums, ferr, caps):
        e = R.rel_err(o[k].np(), want[:n], s[:n])
        bud.check(k + '.cap', float((e / (cap[:n] * R.U32)).max()), 1.0, where)      # per element, in units of its own cap
        frms, fmax = floor_stats(fe, n)
        bud.check(k + '.max', float(e.max()), MAX_X * fmax, where)
        if n >= STAT_MIN_N:
            bud.check(k + '.rms', math.sqrt(float(np.mean(e * e))), RMS_X * frms, where)


STATES = [(coef, t) for coef in R.COEFS for t in (1, 1000)]


@pytest.mark.parametrize('coef, t', STATES, ids=[f'coef{c:.3g}-t{t}' for c, t in STATES])
def test_adamw_dev_against_fp64_and_floor(coef, t):
    ref = wide_ref(coef, t)
    bud = Budget(f'adamw_dev coef={coef:.3g} t={t}')
    full = adamw_call('dev', NWIDE, t, coef)
    for n in sorted(R.ADAMW_SIZES):
        assert R.launch_class(R.plan(L(), R.ADAMW, n), n) == R.ADAMW_SIZES[n]
        outs = []
        for shadow in (True, False):
            o = adamw_call('dev', n, t, coef, shadow=shadow)
            adamw_budget(bud, o, n, ref, (n, shadow))
            outs.append(o)
        assert shadow_is_rne_of_p(outs[0]), n                              # bit for bit, tail included
        assert same_bits(outs[0], outs[1], ('p', 'm', 'v')), n             # the shadow store changes nothing else
        # an element's result does not depend on where the launch puts it: a tail element here is a float4 lane of `full`
        assert all(torch.equal(outs[0][k].t, full[k].t[:n]) for k in ('p', 'm', 'v', 'sh')), n
    bud.done()


@pytest.mark.parametrize('coef, t', STATES, ids=[f'coef{c:.3g}-t{t}' for c, t in STATES])
def test_adamw_host_entry_equals_the_device_state_entry(coef, t):
    """clv_adamw_step without a norm (grad_scale = coef, the same bias corrections) runs the same inlined adam_one."""
    bud = Budget(f'adamw_host coef={coef:.3g} t={t}')
    ref = wide_ref(coef, t)
    for n in sorted(R.ADAMW_SIZES):
        for shadow in (True, False):
            h = adamw_call('host', n, t, coef, shadow=shadow)
            adamw_budget(bud, h, n, ref, (n, shadow))                     # m' and v' of this entry were never looked at
            assert same_bits(h, adamw_call('dev', n, t, coef, shadow=shadow)), (n, shadow)
            assert not shadow or shadow_is_rne_of_p(h)
    bud.done()


@pytest.mark.parametrize('coef, t', STATES, ids=[f'coef{c:.3g}-t{t}' for c, t in STATES])
def test_adamw_16bit_gradient_entry_equals_fp32_entry_on_the_same_values(coef, t):
    p, g, m, v = wide(t)
    g16 = torch.from_numpy(g).to(HALF())
    assert (g16.float() != 0).sum() > NWIDE // 4
    bud = Budget(f'adamw_dev16 coef={coef:.3g} t={t}')
    ref = wide_ref(coef, t, g16=True)
    for n in sorted(R.ADAMW_SIZES):
        a = adamw_call('dev16', n, t, coef, inputs=(p, g16, m, v))
        b = adamw_call('dev', n, t, coef, inputs=(p, g16.float().numpy(), m, v))
        assert same_bits(a, b), n
        adamw_budget(bud, a, n, ref, n)
        assert same_bits(adamw_call('dev16', n, t, coef, inputs=(p, g16, m, v), shadow=False), b, ('p', 'm', 'v')), n
    bud.done()


@pytest.mark.parametrize('entry', ['dev', 'dev16', 'host'])
def test_adamw_exact_properties(entry):
    t, coef = 1000, 0.37
    p, g, m, v = wide(t)
    gin = torch.from_numpy(g).to(HALF()) if entry == 'dev16' else g
    gnz = (torch.as_tensor(gin).float() != 0).numpy()
    for n in (3, 7, 1027):
        # lr = 0: p does not move; m, v and the shadow still do
        o = adamw_call(entry, n, t, coef, lr=0.0, inputs=(p, gin, m, v))
        assert unchanged(o, ('p',)) and shadow_is_rne_of_p(o)
        assert (o['m'].np()[gnz[:n]] != m[:n][gnz[:n]]).all() and (o['v'].np()[gnz[:n]] != v[:n][gnz[:n]]).all()
        # wd = 0 with g = m = 0: nothing to step along, nothing decays
        z = np.zeros_like(g)
        o = adamw_call(entry, n, t, coef, wd=0.0, inputs=(p, torch.from_numpy(z).to(HALF()) if entry == 'dev16' else z, z, v))
        assert unchanged(o, ('p', 'm')) and shadow_is_rne_of_p(o)
        # a skipped step leaves p, m, v AND the shadow alone
        fill = p + 1.0
        if entry == 'host':
            for bad in (math.inf, math.nan):
                o = adamw_call(entry, n, t, coef, sumsq=bad, max_norm=1.0, inputs=(p, gin, m, v), shadow_fill=fill)
                assert unchanged(o, ('p', 'm', 'v', 'sh')), (n, bad)
            # max_norm = 0 with a finite norm: coef is grad_scale, whatever the norm
            o = adamw_call(entry, n, t, coef, sumsq=1e12, max_norm=0.0, inputs=(p, gin, m, v))
            assert same_bits(o, adamw_call('dev', n, t, coef, inputs=(p, gin, m, v)))
        else:
            o = adamw_call(entry, n, t, coef, skip=1, inputs=(p, gin, m, v), shadow_fill=fill)
            assert unchanged(o, ('p', 'm', 'v', 'sh')), n


def test_adamw_host_entry_clips_by_its_norm():
    """The norm branch of clv_adamw_step: coef = grad_scale min(1, max_norm / (sqrt(sumsq grad_scale^2) + 1e-6))."""
    t, n, gs = 1000, 1027, 0.5
    for sumsq, max_norm in ((4.0 * 2 ** 20, 1.0), (4.0, 8.0)):
        norm = np.float32(np.sqrt(np.float32(sumsq * gs * gs)))
        c = np.float32(max_norm) / (norm + np.float32(1e-6))
        coef = float(np.float32(gs) * min(c, np.float32(1.0)))
        o = adamw_call('host', n, t, gs, sumsq=sumsq, max_norm=max_norm)
        assert same_bits(o, adamw_call('dev', n, t, coef)), (sumsq, max_norm)


@pytest.mark.parametrize('entry', ['dev', 'dev16', 'host'])
def test_adamw_refusals_launch_nothing(entry):
    n, t = 1027, 1
    p, g, m, v = wide(t)
    gin = torch.from_numpy(g).to(HALF()) if entry == 'dev16' else g
    cases = [dict(lead={k: 1}) for k in ('p', 'm', 'v', 'sh')] + [dict(lead={'g': 2 if entry == 'dev16' else 1}), dict(n_arg=-1)]
    if entry == 'host':
        cases += [dict(bc1=0.0), dict(bc1=-0.5)]
    for kw in cases:
        o = adamw_call(entry, n, t, 1.0, inputs=(p, gin, m, v), want_rc=-1, **kw)
        assert unchanged(o, ('p', 'm', 'v', 'sh')), kw
    o = adamw_call(entry, n, t, 1.0, inputs=(p, gin, m, v), n_arg=0)              # nothing to do is not an error
    assert unchanged(o, ('p', 'm', 'v', 'sh'))


# ================================================================================================ one chain through ops
def test_chain_through_ops_two_slabs_three_steps_and_a_skip():
    """sumsq_accumulate -> optim_prep -> adamw_step_dev as the engine chains them: slab A (fp32 gradient, with shadow) and
    slab B (16-bit wire gradient written by ops.pack_bf16, no shadow) with different (lr, wd)."""
    from clover_amd import ops
    na, nb, max_norm = 1027, 2050, 1.5
    slabs = [dict(n=na, lr=1e-3, wd=0.05, g16=False, shadow=True), dict(n=nb, lr=2.5e-4, wd=0.0, g16=True, shadow=False)]
    for i, s in enumerate(slabs):
        p = R.wide_state(s['n'], 40 + i, bias(1)[2])[0]
        zero = np.zeros(s['n'], np.float32)
        s.update(p=Guarded(s['n'], values=p), m=Guarded(s['n'], values=zero), v=Guarded(s['n'], values=zero),
                 sh=Guarded(s['n'], HALF(), extra=(-s['n']) % 4) if s['shadow'] else None)
    state, acc = ops.optim_state_new(DEV), Guarded(1, values=[0.0])
    st = R.new_state()
    bud = Budget('chain through ops')
    for step, scale in enumerate([1.0, None, 30.0, 0.01]):
        raw_ref = 0.0
        for i, s in enumerate(slabs):
            g = torch.randn(s['n'], generator=torch.Generator().manual_seed(60 + 10 * step + i)) * (scale or 1.0)
            if scale is None and i == 0:
                g[5] = math.inf
            gd = Guarded(s['n'], values=g)
            if s['g16']:
                g16 = Guarded(s['n'], HALF())
                ops.pack_bf16(gd.t, g16.t)
                assert torch.equal(hbits(g16.t.cpu()), hbits(g.to(HALF()))) and g16.guards_intact()
                gd, g = g16, g.to(HALF()).float()
            s['g'], s['g_ref'] = gd, g.numpy()
            ops.sumsq_accumulate(gd.t, acc.t)
            raw_ref += R.sumsq64(g)
        raw = acc.t.item()                                                  # the very value prep reads
        if scale is not None:
            depth = sum(R.sumsq_depth(R.plan(L(), R.SUMSQ, s['n'])) for s in slabs)
            bud.check('raw.rel', abs(raw - raw_ref) / raw_ref, depth * R.U32, step)
        before = st
        st = R.prep_ref(before, raw, B1, B2, max_norm, 1.0)
        ops.optim_prep(acc.t, state, B1, B2, max_norm, 1.0)
        got = state_read(state)
        prep_compare(got, st, before, bud, step)
        assert acc.t.item() == 0.0 and got['skip'] == int(scale is None)
        rd = ops.optim_state_read(state)
        assert all(rd[k] == got[k] for k in rd)
        for s in slabs:
            old = [s[k].np().astype(np.float64) for k in ('p', 'm', 'v')]
            bits = {k: s[k].bits() for k in ('p', 'm', 'v', 'sh') if s[k] is not None}
            ops.adamw_step_dev(s['p'].t, s['g'].t, s['m'].t, s['v'].t, s['sh'].t if s['sh'] else None, state, s['lr'], B1, B2,
                               EPS, s['wd'])
            torch.cuda.synchronize()
            assert all(s[k].guards_intact() for k in bits)
            if got['skip']:
                assert all(torch.equal(s[k].bits(), b) for k, b in bits.items())
                continue
            args = (got['coef'], got['bc1'], got['bc2_sqrt'], s['lr'], B1, B2, EPS, s['wd'])
            p1, m1, v1, sums = R.adamw64(old[0], s['g_ref'], old[1], old[2], *args)
            fl = R.adamw_floor32(old[0], s['g_ref'], old[1], old[2], *args)
            caps = [R.p_cap(R.cancellation(sums[1], m1)), R.R_M, R.R_V]
            for k, want, sm, f, cap in zip(('p', 'm', 'v'), (p1, m1, v1), sums, fl, caps):
                e, fe = R.rel_err(s[k].np(), want, sm), R.rel_err(f, want, sm)
                bud.check(k + '.cap', float((e / (cap * R.U32)).max()), 1.0, step)
                bud.check(k + '.rms', math.sqrt(float(np.mean(e * e))), RMS_X * math.sqrt(float(np.mean(fe * fe))), step)
                bud.check(k + '.max', float(e.max()), MAX_X * float(fe.max()), step)
            if s['sh']:
                assert torch.equal(hbits(s['sh'].t.cpu()), hbits(s['p'].t.cpu().to(HALF())))
        st = got                                                            # carry the device's own floats forward
    assert st['t'] == 3 and st['skipped'] == 1
    bud.done()


def test_adamw_step_through_ops():
    from clover_amd import ops
    n, t, gs = 1027, 9, 0.37
    p, g, m, v = [a[:n] for a in wide(1000)]
    o = dict(p=Guarded(n, values=p), g=Guarded(n, values=g), m=Guarded(n, values=m), v=Guarded(n, values=v),
             sh=Guarded(n, HALF(), extra=1))
    ops.adamw_step(o['p'].t, o['g'].t, o['m'].t, o['v'].t, o['sh'].t, None, LR, B1, B2, EPS, WD, t, 0.0, grad_scale=gs)
    torch.cuda.synchronize()
    bc1, bc2 = np.float32(1.0 - B1 ** t), np.float32(1.0 - B2 ** t)          # ops computes them in double, the ABI rounds
    args = (R.f32(gs), float(bc1), float(np.sqrt(bc2)), LR, B1, B2, EPS, WD)
    p1, m1, v1, sums = R.adamw64(p, g, m, v, *args)
    fl = R.adamw_floor32(p, g, m, v, *args)
    bud = Budget('adamw_step through ops')
    caps = [R.p_cap(R.cancellation(sums[1], m1)), R.R_M, R.R_V]
    for k, want, sm, f, cap in zip(('p', 'm', 'v'), (p1, m1, v1), sums, fl, caps):
        e, fe = R.rel_err(o[k].np(), want, sm), R.rel_err(f, want, sm)
        bud.check(k + '.cap', float((e / (cap * R.U32)).max()), 1.0)
        bud.check(k + '.rms', math.sqrt(float(np.mean(e * e))), RMS_X * math.sqrt(float(np.mean(fe * fe))))
        bud.check(k + '.max', float(e.max()), MAX_X * float(fe.max()))
    assert shadow_is_rne_of_p(o) and all(o[k].guards_intact() for k in o)
    bud.done()
