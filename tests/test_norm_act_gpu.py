"""Every launch path of csrc/norm_act.hip (LayerNorm vector / scalar kernels with their transforms and gather, the in-kernel
and the batched dgamma / dbeta reduce, the LayerNorm-fold kernels, GELU) against fp64 references, held to what the number
formats alone cost.

tests/norm_ref.py evaluates LayerNorm forward + backward twice per case: with the rounding hook r = identity (the EXACT
reference) and with r = a round trip through the library's 16-bit type (the FLOOR).  16-bit outputs are held to RMS_MARGIN /
ROW_MARGIN times the floor's own error, fp32 outputs to F32_BOUND of the tensor's maximum, and whatever integer arithmetic
makes exact is compared bit for bit.  No bound is fitted to the kernels; the measured figures: tests/NORM_ACT_ERROR_BUDGET.md
(every case prints them as NORM_BUDGET lines under `pytest -s`)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import norm_ref as nr                      # noqa: E402
from clover_amd import _lib                # noqa: E402

DEV = 'cuda'
HALF = _lib.half_dtype()
# kernel error <= margin x floor error: the two margins of tests/test_attention_gpu.py.  Neither may be raised.
RMS_MARGIN, ROW_MARGIN = 2.0, 4.0
# a row whose exact maximum is below this fraction of the tensor's is normalised by this fraction of the tensor's maximum
# (DEGENERATE_SLICE of tests/test_attention_gpu.py)
DEGENERATE_ROW = 1e-3
# fp32 outputs against fp64, max error over the tensor's max: the project's bar for fp32 sinks (tests/test_sinks_gpu.py BOUND,
# tests/test_kernels_gpu.py test_wgrad_accumulates_into_sink)
F32_BOUND = 1e-5
CLV_OK, CLV_ERR_ARG, CLV_ERR_UNSUPPORTED = 0, -1, -2
SEED = 0x1234ABCD9E3779B9                  # the dropout seed of this file: both 32-bit words take part in ln_keep


def ops():
    from clover_amd import ops as o
    return o


def L():
    return _lib.lib()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale


def ints(*shape, lo, hi, seed=0):
    """integer-valued fp32 in [lo, hi]"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device=DEV).float()


def half_rt(t):
    return t.to(HALF).to(t.dtype)


def affine(C_, seed):
    return (1 + 0.1 * rnd(C_, seed=seed + 1)).contiguous(), (0.1 * rnd(C_, seed=seed + 2)).contiguous()


# ----------------------------------------------------------------------------- the C entries
def ln_extra(**kw):
    """ClvLnExtra from keywords; tensors are passed as pointers (the caller keeps them alive)."""
    ex = _lib.ClvLnExtra()
    ex.rows_per_sample = 1
    for k, v in kw.items():
        setattr(ex, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return ex


def _nan_like(t, shape=None):
    return torch.full(shape or t.shape, float('nan'), dtype=t.dtype, device=t.device)


def ln_forward(x, res, gamma, beta, eps, rows, C_, want_sum=False, ex=None, yshape=None):
    """-> rc, dict(y, s, mean, rstd).  Outputs start as NaN: a row the kernel does not write shows."""
    f32 = x.dtype == torch.float32
    y = _nan_like(x, yshape or (rows, C_))
    s = _nan_like(x) if want_sum else None
    mean = torch.full((rows,), float('nan'), device=DEV)
    rstd = mean.clone()
    rc = L().clv_layernorm_fwd(P(x), P(res), P(gamma), P(beta), P(y), P(s), P(mean), P(rstd), rows, C_, float(eps), int(f32),
                               C.byref(ex) if ex is not None else None, stream())
    return rc, dict(y=y, s=s, mean=mean, rstd=rstd)


def ln_backward(dy, x, res, gamma, mean, rstd, dsum, dg, db, rows, C_, ex=None, want_dres=False, deferred=False):
    """dg / db are accumulated into.  deferred: extra.no_reduce, then one clv_ln_reduce_batch entry when the launch left
    partials — the route of every large LayerNorm inside a backward segment.  -> rc, dict(dx, dres)"""
    f32 = x.dtype == torch.float32
    nblk = L().clv_layernorm_bwd_blocks(rows, C_)
    partial = torch.full((2 * nblk * C_,), float('nan'), device=DEV)
    dx = _nan_like(x)
    dres = _nan_like(x) if want_dres else None
    if want_dres or deferred:
        ex = ex if ex is not None else ln_extra()
        ex.dres = dres.data_ptr() if want_dres else None
        ex.no_reduce = int(deferred)
    rc = L().clv_layernorm_bwd(P(dy), P(x), P(res), P(gamma), P(mean), P(rstd), P(dsum), P(dx), P(dg), P(db), P(partial),
                               rows, C_, int(f32), C.byref(ex) if ex is not None else None, stream())
    if rc == CLV_OK and deferred and L().clv_layernorm_bwd_needs_reduce(rows, C_):
        ent = (_lib.ClvLnReduceEntry * 1)()
        ent[0].partial, ent[0].dgamma, ent[0].dbeta, ent[0].nblk, ent[0].C = partial.data_ptr(), dg.data_ptr(), \
            db.data_ptr(), nblk, C_
        rc = L().clv_ln_reduce_batch(ent, 1, stream())
    torch.cuda.synchronize()
    return rc, dict(dx=dx, dres=dres)


# ----------------------------------------------------------------------------- the assertions
def rms_err(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-300)).item()


def row_err(a, b):
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    norm = b.abs().amax(1).clamp_min(DEGENERATE_ROW * b.abs().max()).clamp_min(1e-300)
    return ((a - b).abs().amax(1) / norm).max().item()


def max_err(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _ratio(k, f):
    return k / f if f > 0 else (0.0 if k == 0 else float('inf'))


def hold(case, got, exact, floor, f32, mixed=()):
    """got / exact / floor: dicts of tensors; None entries of `got` are outputs the case does not produce.  16-bit storage:
    y, s, dx, dres are held to the floor, mean / rstd / dgamma / dbeta to F32_BOUND; a name in `mixed` (dgamma of a backward
    that re-read the stored sum) passes either.  fp32 storage: everything to F32_BOUND.  Prints, then asserts all at once."""
    bad = []
    for name, g in got.items():
        if g is None:
            continue
        e = exact[name]
        g = g.double().reshape(e.shape)
        assert torch.isfinite(g).all(), f'{case} {name}: non-finite values (or rows that were never written)'
        me = max_err(g, e)
        to_floor = not f32 and (name in ('y', 's', 'dx', 'dres') or name in mixed)
        if not to_floor:
            print(f'NORM_BUDGET | {case} | {name} | fp32 max/max {me:.2e}')
            if me > F32_BOUND:
                bad.append(f'{name}: max error {me:.3e} of the maximum (allowed {F32_BOUND})')
            continue
        f = floor[name]
        e2, g2, f2 = (t if t.dim() > 1 else t[None] for t in (e, g, f))
        fr, kr, fs, ks = rms_err(f2, e2), rms_err(g2, e2), row_err(f2, e2), row_err(g2, e2)
        print(f'NORM_BUDGET | {case} | {name} | floor rms {fr:.3e} kernel/floor {_ratio(kr, fr):.2f} | floor row {fs:.3e} '
              f'kernel/floor {_ratio(ks, fs):.2f} | max/max {me:.2e}')
        if name in mixed and me <= F32_BOUND:
            continue
        if kr > RMS_MARGIN * fr:
            bad.append(f'{name}: RMS error {kr:.3e} = {_ratio(kr, fr):.2f} x floor {fr:.3e} (allowed {RMS_MARGIN})')
        if ks > ROW_MARGIN * fs:
            bad.append(f'{name}: row error {ks:.3e} = {_ratio(ks, fs):.2f} x floor {fs:.3e} (allowed {ROW_MARGIN})')
    assert not bad, f'{case}: ' + '; '.join(bad)


# ----------------------------------------------------------------------------- one LayerNorm case, forward + backward
def check_ln(case, rows, C_, *, f32=False, with_res=False, x_is_sum=False, with_dsum=False, with_dy2=False, scale=None,
             drop_p=0.0, int_dy=False, eps=1e-5, routes=(False,), seed=0, forward_only=False):
    """Inputs: seeded randn rounded to the 16-bit type (stored as fp32 for the fp32 instantiation); gamma = 1 + 0.1 randn,
    beta = 0.1 randn.  scale: per-sample factors (rows split evenly); drop_p: dropout on x with SEED.  x_is_sum: the forward
    also stores the sum and the backward reads THAT (extra.x_is_sum) — the route of a LayerNorm that returns its sum.
    int_dy: integer upstream gradients in [-8, 8] — dbeta is then exact in any summation order.  routes: for each entry the
    backward runs once, False = reduce inside clv_layernorm_bwd, True = no_reduce + clv_ln_reduce_batch."""
    st = torch.float32 if f32 else HALF
    store = lambda t: None if t is None else t.to(HALF).to(st).contiguous()      # noqa: E731
    x = store(rnd(rows, C_, seed=seed + 10))
    res = store(rnd(rows, C_, seed=seed + 11)) if with_res else None
    dy = store(ints(rows, C_, lo=-8, hi=8, seed=seed + 12) if int_dy else rnd(rows, C_, seed=seed + 12))
    dy2 = store(rnd(rows, C_, seed=seed + 13)) if with_dy2 else None
    dsum = store(rnd(rows, C_, seed=seed + 14)) if with_dsum else None
    gamma, beta = affine(C_, seed + 20)
    kw, keep_alive, k = {}, [], None
    if scale is not None:
        xs = torch.tensor(scale, device=DEV, dtype=torch.float32)
        rps = rows // len(scale)
        assert rps * len(scale) == rows
        kw.update(xscale=xs, rows_per_sample=rps)
        keep_alive.append(xs)
        k = xs.repeat_interleave(rps)[:, None].expand(rows, C_)
    if drop_p:
        sd = torch.tensor([SEED], dtype=torch.int64, device=DEV)
        kw.update(drop_p=float(drop_p), seed=sd)
        keep_alive.append(sd)
        km = nr.ln_keep_mask(SEED, rows, C_, drop_p, device=DEV).float() * nr.inv_keep(drop_p)
        k = km if k is None else k * km          # fp32, as the kernel multiplies them
    rc, fw = ln_forward(x, res, gamma, beta, eps, rows, C_, want_sum=x_is_sum, ex=ln_extra(**kw) if kw else None)
    assert rc == CLV_OK, (case, rc)
    torch.cuda.synchronize()
    r = nr.ident if f32 else half_rt
    args = (x, res, k, gamma, beta, eps, dy, dy2, dsum)
    exact = nr.ln_core(*args, nr.ident, x_is_sum)
    floor = exact if f32 else nr.ln_core(*args, r, x_is_sum)
    if forward_only:
        hold(case + ' fwd', fw, exact, floor, f32)
        return
    dg0, db0 = ints(C_, lo=-4, hi=4, seed=seed + 30), ints(C_, lo=-4, hi=4, seed=seed + 31)     # the accumulators' start
    want_dres = k is not None and with_res           # (as ops._LayerNorm: the two gradients differ only then)
    for deferred in routes:
        dg, db = dg0.clone(), db0.clone()
        bkw = dict(kw, x_is_sum=int(x_is_sum), dy2=dy2) if (kw or x_is_sum or dy2 is not None) else {}
        rc, bw = ln_backward(dy, fw['s'] if x_is_sum else x, None if x_is_sum else res, gamma, fw['mean'], fw['rstd'], dsum,
                             dg, db, rows, C_, ex=ln_extra(**{a: b for a, b in bkw.items() if b is not None}) if bkw else None,
                             want_dres=want_dres, deferred=deferred)
        assert rc == CLV_OK, (case, rc)
        tag = case + (' deferred' if deferred else '')
        if int_dy:
            want = (dy.double().sum(0) + db0.double()).float()
            assert torch.equal(db, want), f'{tag}: dbeta of integer gradients is not exact: {(db - want).abs().max().item()}'
        if k is not None:
            dead = (k == 0).expand(rows, C_)
            assert (exact['dx'][dead] == 0).all()
            assert (bw['dx'][dead] == 0).all(), f'{tag}: dx is not zero where the multiplier on x is zero'
        # the accumulators must hold start + gradient: result - start (exact in fp64) is compared with the gradient, so the
        # error is that of the sum and the scale is the gradient's
        got = dict(fw, dgamma=dg.double() - dg0.double(), dbeta=db.double() - db0.double(), **bw)
        hold(tag, got, exact, floor, f32, mixed=('dgamma',) if x_is_sum else ())
    del keep_alive


# width classes: every (group, iters) pair of lnv_config, ragged last chunks, the classes' upper ends; * = also fp32 storage
VECTOR_WIDTHS = [(8, 1), (48, 0), (104, 0), (128, 0), (136, 0), (200, 1), (256, 0), (264, 0), (512, 0), (520, 1), (1024, 0),
                 (1032, 0), (1544, 0), (2056, 0), (3072, 1)]
SCALAR_WIDTHS = [(2, 0), (100, 1), (130, 0), (258, 0), (3080, 0), (4096, 0)]
WIDTH_CASES = [(c, False) for c, _ in VECTOR_WIDTHS + SCALAR_WIDTHS] + [(c, True) for c, s in VECTOR_WIDTHS + SCALAR_WIDTHS if s]


@pytest.mark.parametrize('C_,f32', WIDTH_CASES, ids=[f'C{c}{"-f32" if f else ""}' for c, f in WIDTH_CASES])
@pytest.mark.parametrize('stream_sum', [False, True], ids=['plain', 'res-sum-dsum'])
def test_width_classes(C_, f32, stream_sum):
    """37 rows of every width class: plain, and with a residual operand, the stored sum re-read by the backward, and a
    gradient arriving on the sum."""
    check_ln(f'width C={C_} {"f32" if f32 else "16"} {"sum" if stream_sum else "plain"}', 37, C_, f32=f32, with_res=stream_sum,
             x_is_sum=stream_sum, with_dsum=stream_sum, seed=C_)


def test_small_eps():
    check_ln('eps 1e-12 C=264', 37, 264, eps=1e-12, with_res=True, x_is_sum=True, with_dsum=True, seed=5)
    check_ln('eps 1e-12 C=100', 37, 100, eps=1e-12, seed=6)


# (rows, C, expected clv_layernorm_bwd_blocks, expected needs_reduce).  rows per block: 16 (group 16), 8 (group 32), 4 (group
# 64 and the scalar kernels); caps: 768 where three row groups are in flight (groups 16 / 32), 1280 for group 64 with one
# chunk per lane, 512 with several, 2048 for the scalar kernels.  x against x + 1 rows: 256 against 257 blocks (direct atomics
# against partials + reduce), the first row beyond a cap, and at 36865 rows the second trip of the three-groups loop.
ROW_CASES = [(1, 8, 1, 0), (15, 8, 1, 0), (17, 8, 2, 0), (4096, 8, 256, 0), (4097, 8, 257, 1), (12289, 8, 768, 1),
             (36865, 8, 768, 1), (36865, 128, 768, 1),
             (2048, 136, 256, 0), (2049, 136, 257, 1), (6145, 136, 768, 1),
             # group 32's third row group in flight starts at row 2 x 768 x 8 = 12288 (group 16's: 24576, inside 36865 rows)
             (12289, 136, 768, 1),
             (1024, 264, 256, 0), (1025, 264, 257, 1), (5121, 264, 1280, 1),
             (1024, 520, 256, 0), (1025, 520, 257, 1), (2049, 520, 512, 1),
             (1024, 100, 256, 0), (1025, 100, 257, 1), (8193, 100, 2048, 1)]


@pytest.mark.parametrize('rows,C_,blocks,reduce', ROW_CASES, ids=[f'{r}x{c}' for r, c, _, _ in ROW_CASES])
@pytest.mark.parametrize('int_dy', [True, False], ids=['int-dy', 'rand-dy'])
def test_row_accounting(rows, C_, blocks, reduce, int_dy):
    """Every row counted once, on both sides of every grid boundary, by both reduce routes."""
    assert L().clv_layernorm_bwd_blocks(rows, C_) == blocks
    assert L().clv_layernorm_bwd_needs_reduce(rows, C_) == reduce
    check_ln(f'rows {rows}x{C_} {"int" if int_dy else "rand"}', rows, C_, int_dy=int_dy, routes=(False, True) if reduce else (False,),
             seed=rows + C_)


@pytest.mark.parametrize('int_dy', [True, False], ids=['int-dy', 'rand-dy'])
def test_row_accounting_fp32_instantiation(int_dy):
    """fp32 storage keeps the plain loop under the cap of the three-groups kernels."""
    assert L().clv_layernorm_bwd_blocks(12289, 8) == 768
    check_ln(f'rows 12289x8 f32 {"int" if int_dy else "rand"}', 12289, 8, f32=True, int_dy=int_dy, routes=(False, True), seed=3)


def test_scalar_forward_second_trip():
    """8193 rows = 2049 blocks of 4 waves against the scalar forward's 2048-block grid."""
    check_ln('scalar fwd 8193x100', 8193, 100, with_res=True, x_is_sum=True, forward_only=True, seed=9)


# ----------------------------------------------------------------------------- operand transforms
@pytest.mark.parametrize('C_', [8, 136, 264, 520])
@pytest.mark.parametrize('with_res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('x_is_sum', [False, True], ids=['raw', 'sum'])
def test_transforms(C_, with_res, x_is_sum):
    """Per-sample scale [0, 1.25, 1.25, 0] and dropout 0.2 on x, 4 samples x 50 rows, a second upstream gradient, dres when
    the residual's gradient differs from dx."""
    kw = dict(with_res=with_res, x_is_sum=x_is_sum, with_dsum=x_is_sum, with_dy2=True, seed=C_ + 1)
    tag = f'xform C={C_} {"res" if with_res else "nores"} {"sum" if x_is_sum else "raw"}'
    check_ln(tag + ' scale+drop', 200, C_, scale=[0.0, 1.25, 1.25, 0.0], drop_p=0.2, **kw)
    check_ln(tag + ' scale', 200, C_, scale=[0.0, 1.25, 1.25, 0.0], **kw)
    check_ln(tag + ' drop', 200, C_, drop_p=0.2, **kw)


@pytest.mark.parametrize('rows,C_', [(200, 8), (200, 136), (200, 264), (200, 520), (36865, 8)])
def test_dropout_mask_is_ln_keep(rows, C_):
    """An all-ones operand: the stored sum is keep / (1 - p), so the kernel's mask can be read off and compared with the
    integer restatement of ln_keep."""
    p = 0.2
    x = torch.ones(rows, C_, device=DEV, dtype=HALF)
    gamma, beta = affine(C_, 1)
    sd = torch.tensor([SEED], dtype=torch.int64, device=DEV)
    rc, fw = ln_forward(x, None, gamma, beta, 1e-5, rows, C_, want_sum=True, ex=ln_extra(drop_p=p, seed=sd))
    assert rc == CLV_OK
    torch.cuda.synchronize()
    want = nr.ln_keep_mask(SEED, rows, C_, p, device=DEV)
    assert torch.equal(fw['s'] != 0, want)
    assert torch.equal(fw['s'], (want.float() * nr.inv_keep(p)).to(HALF))
    n = rows * C_
    assert abs(want.double().mean().item() - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5


# ----------------------------------------------------------------------------- PatchMerging gather
@pytest.mark.parametrize('shape', [(1, 1, 2, 2, 8), (2, 3, 6, 10, 32), (2, 2, 28, 28, 96)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('with_res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('with_scale', [False, True], ids=['noscale', 'scale'])
def test_gather(shape, with_res, with_scale):
    B, D, H, W, Cs = shape
    H2, W2, C4 = H // 2, W // 2, 4 * Cs
    rows = B * D * H2 * W2
    case = f'gather {"x".join(map(str, shape))} {"res" if with_res else "nores"} {"scale" if with_scale else "noscale"}'
    x = rnd(*shape, seed=41).to(HALF)
    res = rnd(*shape, seed=42).to(HALF) if with_res else None
    dy = rnd(rows, C4, seed=43).to(HALF)
    gamma, beta = affine(C4, 44)
    xs = torch.tensor([0.0, 1.25][-B:], device=DEV) if with_scale else None
    kw = dict(gather_c=Cs, gather_h2=H2, gather_w2=W2, rows_per_sample=D * H2 * W2)
    if with_scale:
        kw['xscale'] = xs
    rc, fw = ln_forward(x, res, gamma, beta, 1e-5, rows, C4, ex=ln_extra(**kw), yshape=(rows, C4))
    assert rc == CLV_OK
    dg0, db0 = ints(C4, lo=-4, hi=4, seed=45), ints(C4, lo=-4, hi=4, seed=46)
    dg, db = dg0.clone(), db0.clone()
    want_dres = with_scale and with_res
    rc, bw = ln_backward(dy, x, res, gamma, fw['mean'], fw['rstd'], None, dg, db, rows, C4, ex=ln_extra(**kw), want_dres=want_dres)
    assert rc == CLV_OK
    k5 = xs.view(B, 1, 1, 1, 1).expand(shape) if with_scale else None
    args = (nr.merge_gather(x), nr.merge_gather(res) if with_res else None, nr.merge_gather(k5) if with_scale else None,
            gamma, beta, 1e-5, dy, None, None)
    exact, floor = nr.ln_core(*args, nr.ident, False), nr.ln_core(*args, half_rt, False)
    # dx / dres come back in the un-gathered layout, every element written once (they start as NaN): compare gathered
    got = dict(y=fw['y'], mean=fw['mean'], rstd=fw['rstd'], dgamma=dg.double() - dg0.double(),
               dbeta=db.double() - db0.double(), dx=nr.merge_gather(bw['dx']),
               dres=nr.merge_gather(bw['dres']) if want_dres else None)
    if with_scale and B > 1:
        assert (bw['dx'][0] == 0).all(), f'{case}: dx is not zero on the sample whose scale is 0'
    hold(case, got, exact, floor, False)


# ----------------------------------------------------------------------------- deferred reduce
REDUCE_PAIRS = [(1, 8), (257, 8), (300, 100), (2048, 264), (512, 3072)]


@pytest.mark.parametrize('n', [1, 3, _lib.LN_REDUCE_MAX])
def test_reduce_batch_is_exact_on_integers(n):
    """clv_ln_reduce_batch on integer partials into non-zero targets: any order of fp32 adds is exact."""
    arr = (_lib.ClvLnReduceEntry * n)()
    keep = []
    for i in range(n):
        nblk, C_ = REDUCE_PAIRS[3] if n == 1 else REDUCE_PAIRS[i % len(REDUCE_PAIRS)]
        part = ints(2, nblk, C_, lo=-8, hi=8, seed=100 + i)
        dg0, db0 = ints(C_, lo=-64, hi=64, seed=200 + i), ints(C_, lo=-64, hi=64, seed=300 + i)
        dg, db = dg0.clone(), db0.clone()
        arr[i].partial, arr[i].dgamma, arr[i].dbeta, arr[i].nblk, arr[i].C = part.data_ptr(), dg.data_ptr(), db.data_ptr(), nblk, C_
        keep.append((part, dg0, db0, dg, db))
    assert L().clv_ln_reduce_batch(arr, n, stream()) == CLV_OK
    torch.cuda.synchronize()
    for i, (part, dg0, db0, dg, db) in enumerate(keep):
        s = part.double().sum(1)
        assert torch.equal(dg, (dg0.double() + s[0]).float()), f'entry {i} {tuple(part.shape)}: dgamma'
        assert torch.equal(db, (db0.double() + s[1]).float()), f'entry {i} {tuple(part.shape)}: dbeta'
    assert L().clv_ln_reduce_batch(arr, 0, stream()) == CLV_ERR_ARG
    assert L().clv_ln_reduce_batch(arr, _lib.LN_REDUCE_MAX + 1, stream()) == CLV_ERR_ARG


def test_deferred_reduce_through_ops():
    """Two ops.layer_norm backwards with sinks inside ops.defer_folds(): both leave an entry in the segment, and the sinks
    hold what the undeferred backward delivers."""
    o = ops()
    shapes = [(4097, 8), (1025, 264)]
    data = []
    for i, (rows, C_) in enumerate(shapes):
        gamma, beta = affine(C_, 50 + i)
        data.append((rnd(rows, C_, seed=60 + i).to(HALF), rnd(rows, C_, seed=70 + i).to(HALF), gamma, beta,
                     ints(C_, lo=-4, hi=4, seed=80 + i), ints(C_, lo=-4, hi=4, seed=90 + i)))

    def run(defer):
        params, outs, ready = [], [], []
        for x, dy, gamma, beta, dg0, db0 in data:
            g, b = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
            g._clv_grad, b._clv_grad = dg0.clone(), db0.clone()
            g._clv_ready = b._clv_ready = lambda: ready.append(1)
            params.append((g, b))
            outs.append((o.layer_norm(x.clone().requires_grad_(), g, b), dy))
        if defer:
            with o.defer_folds():
                for y, dy in outs:
                    y.backward(dy)
                assert len(o.SEGMENT.ln_reduces) == 2
                assert [(it.nblk, it.C) for it in o.SEGMENT.ln_reduces] == [(257, 8), (257, 264)]
            assert o.SEGMENT is None
        else:
            for y, dy in outs:
                y.backward(dy)
        torch.cuda.synchronize()
        assert len(ready) == 4 and all(g.grad is None and b.grad is None for g, b in params)
        return [(g._clv_grad, b._clv_grad) for g, b in params]

    plain, deferred = run(False), run(True)
    for (rows, C_), (x, dy, gamma, beta, dg0, db0), pl, de in zip(shapes, data, plain, deferred):
        exact = nr.ln_core(x, None, None, gamma, beta, 1e-5, dy, None, None, nr.ident, False)
        for name, start, a, b in (('dgamma', dg0, pl[0], de[0]), ('dbeta', db0, pl[1], de[1])):
            ref = exact[name]
            e_routes = ((b.double() - a.double()).abs().max() / ref.abs().max()).item()
            e_ref = ((b.double() - start.double() - ref).abs().max() / ref.abs().max()).item()
            print(f'NORM_BUDGET | deferred ops {rows}x{C_} | {name} | fp32 max/max {e_ref:.2e} (against undeferred {e_routes:.2e})')
            assert e_routes <= F32_BOUND and e_ref <= F32_BOUND, (rows, C_, name, e_routes, e_ref)


# ----------------------------------------------------------------------------- argument returns (no launch)
def test_argument_returns():
    def call(rows, C_, ex=None, f32=False):
        """-> (forward rc, backward rc, y) on real buffers of the stated shape"""
        st = torch.float32 if f32 else HALF
        n = max(rows, 1)
        x = torch.ones(n, C_, device=DEV, dtype=st)
        gamma, beta = torch.ones(C_, device=DEV), torch.zeros(C_, device=DEV)
        rc_f, fw = ln_forward(x, None, gamma, beta, 1e-5, rows, C_, ex=ex, yshape=(n, C_))
        dg, db = torch.zeros(C_, device=DEV), torch.zeros(C_, device=DEV)
        mean, rstd = torch.zeros(n, device=DEV), torch.ones(n, device=DEV)
        nblk = max(L().clv_layernorm_bwd_blocks(n, C_), 1)
        partial = torch.zeros(2 * nblk * C_, device=DEV)
        dx = torch.full_like(x, float('nan'))
        rc_b = L().clv_layernorm_bwd(P(x), P(x), None, P(gamma), P(mean), P(rstd), None, P(dx), P(dg), P(db), P(partial), rows,
                                     C_, int(f32), C.byref(ex) if ex is not None else None, stream())
        torch.cuda.synchronize()
        if rc_f != CLV_OK or rows == 0:           # a refused call, or one without rows, writes nothing
            assert torch.isnan(fw['y']).all()
        if rc_b != CLV_OK:
            assert torch.isnan(dx).all()
        return rc_f, rc_b

    xs = torch.ones(2, device=DEV)
    for f32 in (False, True):
        assert call(4, 7, f32=f32) == (CLV_ERR_ARG, CLV_ERR_ARG)                                  # odd C
        assert call(2, 4098, f32=f32) == (CLV_ERR_UNSUPPORTED, CLV_ERR_UNSUPPORTED)               # beyond the widest kernel
        # the scalar fallback has no operand transforms
        assert call(4, 100, ln_extra(xscale=xs, rows_per_sample=2), f32) == (CLV_ERR_UNSUPPORTED, CLV_ERR_UNSUPPORTED)
        assert call(4, 64, ln_extra(gather_c=8, gather_h2=2, gather_w2=2), f32) == (CLV_ERR_ARG, CLV_ERR_ARG)   # 4 gather_c != C
        assert call(4, 64, ln_extra(drop_p=0.2), f32) == (CLV_ERR_ARG, CLV_ERR_ARG)               # dropout without a seed
        assert call(0, 64, f32=f32)[0] == CLV_OK                                                  # no rows


# ----------------------------------------------------------------------------- LayerNorm fold
@pytest.mark.parametrize('N,K', [(1, 8), (5, 96), (7, 129), (288, 96), (30, 300)])
@pytest.mark.parametrize('with_b', [False, True], ids=['nob', 'b'])
def test_ln_fold(N, K, with_b):
    """wf = half(w gamma) exactly (one multiply, one round to nearest even), bf = b + w beta; the backward adds into four
    accumulators that start non-zero (4-row block tail at N % 4, K loop of stride 128 at K = 129 / 300)."""
    case = f'fold {N}x{K} {"b" if with_b else "nob"}'
    w, b = rnd(N, K, scale=0.1, seed=1).contiguous(), (rnd(N, scale=0.1, seed=2) if with_b else None)
    gamma, beta = affine(K, 3)
    wf = torch.full((N, K), float('nan'), device=DEV, dtype=HALF)
    bf = torch.full((N,), float('nan'), device=DEV)
    assert L().clv_ln_fold_fwd(P(w), P(b), P(gamma), P(beta), P(wf), P(bf), N, K, stream()) == CLV_OK
    torch.cuda.synchronize()
    assert torch.equal(wf, (w * gamma).to(HALF)), f'{case}: wf is not half(w * gamma)'
    bf_ref = (b.double() if with_b else 0.0) + w.double() @ beta.double()
    dwf, dbf = rnd(N, K, seed=4).contiguous(), rnd(N, seed=5)
    start = dict(dw=rnd(N, K, seed=6).contiguous(), db=rnd(N, seed=7), dgamma=rnd(K, seed=8), dbeta=rnd(K, seed=9))
    acc = {n: t.clone() for n, t in start.items()}
    assert L().clv_ln_fold_bwd(P(dwf), P(dbf), P(w), P(gamma), P(beta), P(acc['dw']), P(acc['db']) if with_b else None,
                               P(acc['dgamma']), P(acc['dbeta']), N, K, stream()) == CLV_OK
    torch.cuda.synchronize()
    grad = dict(dw=dwf.double() * gamma.double() + dbf.double()[:, None] * beta.double(), db=dbf.double(),
                dgamma=(dwf.double() * w.double()).sum(0), dbeta=(dbf.double()[:, None] * w.double()).sum(0))
    bad = []
    e = max_err(bf.double(), bf_ref)
    print(f'NORM_BUDGET | {case} | bf | fp32 max/max {e:.2e}')
    if e > F32_BOUND:
        bad.append(f'bf {e:.3e}')
    for name, g in grad.items():
        if name == 'db' and not with_b:
            assert torch.equal(acc['db'], start['db'])          # not passed: untouched
            continue
        e = ((acc[name].double() - start[name].double() - g).abs().max() / g.abs().max()).item()
        print(f'NORM_BUDGET | {case} | {name} | fp32 max/max {e:.2e}')
        if e > F32_BOUND:
            bad.append(f'{name} {e:.3e}')
    assert not bad, f'{case}: beyond {F32_BOUND} of the maximum: ' + ', '.join(bad)


# ----------------------------------------------------------------------------- GELU
def finite_values():
    """Every finite value of the 16-bit type, in a seeded random order (a short tensor then holds typical values)."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(HALF)
    v = bits[torch.isfinite(bits)]
    return v[torch.randperm(v.numel(), generator=torch.Generator().manual_seed(7))].to(DEV)


def gelu_bounds(x):
    """3e-7: the polynomial's documented 1.5e-7 in erf (common.hpp), halved in Phi, plus three fp32 roundings of 2^-24."""
    x64 = x.double()
    return nr.gelu64(x64), 3e-7 * x64.abs(), nr.gelu_grad64(x64), 3e-7 * (1 + x64.abs())


def _gelu_assert(case, got, ref, allow):
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all(), f'{case}: non-finite values'
    worst = (err / allow.clamp_min(1e-300)).max().item()
    print(f'NORM_BUDGET | {case} | error / allowance {worst:.3f}')
    i = int((err - allow).argmax())
    assert (err <= allow).all(), f'{case}: |error| {err[i].item():.3e} > {allow[i].item():.3e} at value {ref[i].item():.6e} ({worst:.2f} x)'


@pytest.mark.parametrize('n', [1, 7, 8, 9, 2053, 65541])
def test_gelu_16bit(n):
    """ops.gelu forward, and backward with dy = 1, over every finite value of the 16-bit type; lengths around the 8-element
    groups (the n - 8 * (n // 8) tail runs at every length but 8).  Allowance: one 16-bit rounding of a value within 3e-7."""
    vals = finite_values()
    x = vals[torch.arange(n, device=DEV) % vals.numel()].contiguous()
    y_ref, y_tol, g_ref, g_tol = gelu_bounds(x)
    xr = x.clone().requires_grad_()
    y = ops().gelu(xr)
    y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    assert y.dtype == HALF and xr.grad.dtype == HALF and y.shape == x.shape
    _gelu_assert(f'gelu fwd n={n}', y.detach(), y_ref, nr.spacing16(y_ref, HALF) + y_tol)
    _gelu_assert(f'gelu bwd n={n}', xr.grad, g_ref, nr.spacing16(g_ref, HALF) + g_tol)


@pytest.mark.parametrize('n', [1, 7, 8, 9, 2053, 65541])
def test_gelu_fp32_entries(n):
    """clv_gelu_fwd / clv_gelu_bwd with is_f32 over the same values; 2^-23 |value| takes the place of the 16-bit spacing."""
    vals = finite_values()
    x = vals[torch.arange(n, device=DEV) % vals.numel()].float().contiguous()
    y_ref, y_tol, g_ref, g_tol = gelu_bounds(x)
    y, dx = torch.full_like(x, float('nan')), torch.full_like(x, float('nan'))
    guard = torch.ones_like(x)
    assert L().clv_gelu_fwd(P(x), P(y), n, 1, stream()) == CLV_OK
    assert L().clv_gelu_bwd(P(guard), P(x), P(dx), n, 1, stream()) == CLV_OK
    torch.cuda.synchronize()
    _gelu_assert(f'gelu f32 fwd n={n}', y, y_ref, 2.0 ** -23 * y_ref.abs() + y_tol)
    _gelu_assert(f'gelu f32 bwd n={n}', dx, g_ref, 2.0 ** -23 * g_ref.abs() + g_tol)
