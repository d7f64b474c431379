"""Every launch class of csrc/gemm_wgrad.hip through the C entries, bit-exact on integer data.

The stand-alone kernels (in place, partial + fold in plain and in XCD-mapped block order, standardise-on-load), the grouped
launch of both tile classes, the two fold kernels with 1, 4 and 16 slice-lanes, the norm slots and clv_colsum run on the
integer inputs of tests/wgrad_ref.py, whose caps make fp32 accumulation independent of its order: results are compared with
torch.equal against the int64 reference.  Every case first asserts, through the library's host entries, the planning facts it
was written for (slice count, slice length, the rows of the last slices — one, none, or a negative count —, tile class, in
place or not, lanes of the fold): a retuned planner fails here instead of moving the case to another path.

Buffers: whatever a kernel STORES starts as NaN (partials, first-touch dW, fresh db), whatever it ACCUMULATES into starts as
integers; operands carry NaN in their padding columns and in GUARD_ROWS rows past M, outputs and partials a NaN tail that
must still be NaN afterwards — a read past a slice's end or a write past a buffer's shows in the comparison instead of in
somebody else's memory.

One random-data case per kernel family holds the kernels to two bounds that are not fitted to them (test_random_data); the
measured ratios: tests/WGRAD_ERROR_BUDGET.md (WGRAD_BUDGET lines under `pytest -s`)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import wgrad_ref as wr                     # noqa: E402
from clover_amd import _lib                # noqa: E402

DEV = 'cuda'
HALF = _lib.half_dtype()
NAN = float('nan')
GUARD_ROWS = 64                            # operand rows past M (two stages: what a missing row bound would read)
SLOTS, SLOT_STRIDE = 64, 16                # CLV_SUMSQ_SLOTS accumulators, 16 floats apart
# fp32 sinks against fp64, max error over the tensor's max: the project's bar (tests/test_norm_act_gpu.py F32_BOUND,
# tests/test_kernels_gpu.py test_wgrad_accumulates_into_sink).  Not to be raised.
F32_BOUND = 1e-5
# unit roundoff of the per-element summation bound: 2^-23, not 2^-24 — whether the matrix unit's fp32 accumulate rounds to
# nearest or truncates has not been verified, and the bound must hold either way
U = 2.0 ** -23


def L():
    return _lib.lib()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- guarded buffers
class Operand:
    """A 16-bit operand [M][W] as a column slice of a wider NaN-filled tensor with GUARD_ROWS NaN rows after it."""

    def __init__(self, t, pad=0, off=0):
        M, W = t.shape
        assert pad % 8 == 0 and off % 8 == 0 and off <= pad
        self.buf = torch.full((M + GUARD_ROWS, W + pad), NAN, dtype=HALF, device=DEV)
        self.view = self.buf[:M, off:off + W]
        self.view.copy_(t)
        self.before = self.buf.clone()
        self.ld = W + pad

    def ptr(self):
        return self.view.data_ptr()

    def check(self, what):
        assert torch.equal(self.buf.view(torch.int16), self.before.view(torch.int16)), f'{what}: an operand was written'


class Out:
    """fp32 output / work buffer of n floats (fill: a CPU tensor, or a number) followed by a NaN tail."""

    def __init__(self, n, fill, tail=4096):
        self.n = n
        self.buf = torch.full((n + tail,), NAN, dtype=torch.float32, device=DEV)
        if isinstance(fill, torch.Tensor):
            self.buf[:n].copy_(fill.reshape(-1))
        else:
            self.buf[:n].fill_(fill)
        self.t = self.buf[:n]

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, what):
        assert torch.isnan(self.buf[self.n:]).all(), f'{what}: written past its end'


def eq(got, ref64, what):
    """bit-exact: got (fp32, device) against an int64 reference"""
    g = got.detach().cpu().reshape(ref64.shape)
    if not torch.equal(g, ref64.float()):
        bad = (g != ref64.float()) | torch.isnan(g)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference '
                             f'({int(torch.isnan(g).sum())} NaN), first at {idx}: got {g[tuple(idx)].item()}, '
                             f'exact {ref64[tuple(idx)].item()}')


def work_out(splits, E2):
    return Out(splits * E2, NAN, tail=8 * E2 + 4096)          # 7 more slabs: what the padding blocks of an XCD-mapped grid would hit


def check_partials(work, splits, N, K, case, bias, what):
    """The slabs of a partial launch: every dW element of every slab written, their sum the exact dy^T x; the db part
    likewise with bias, untouched (NaN) without."""
    w = work.t.view(splits, N * K + N)
    eq(w[:, :N * K].sum(0), case.dw_first, f'{what}: sum of the partial slabs')
    if bias:
        eq(w[:, N * K:].sum(0), case.db - case.db0.long(), f'{what}: sum of the partial bias slabs')
    else:
        assert torch.isnan(w[:, N * K:]).all(), f'{what}: bias partials written without want_bias'
    work.check(f'{what}: partial buffer')


# ----------------------------------------------------------------------------- stand-alone clv_linear_wgrad
def run_single(M, N, K, case, split_stages, bias, pad=(0, 0), off=(0, 0), what=''):
    splits = L().clv_linear_wgrad_splits(M, N, K)
    E2 = N * K + N
    stats = case.mean is not None
    dy, x = Operand(case.dy, pad[0], off[0]), Operand(case.x, pad[1], off[1])
    dw, db = Out(N * K, case.dw0), Out(N, case.db0)
    work = work_out(splits, E2)
    mean = rstd = None
    if stats:
        mean, rstd = Out(M, case.mean, tail=GUARD_ROWS), Out(M, case.rstd, tail=GUARD_ROWS)
    args = (C.c_void_p(dy.ptr()), C.c_void_p(x.ptr()), P(dw.buf), P(db.buf) if bias else None, P(work.buf), M, N, K, dy.ld,
            x.ld, P(mean.buf) if stats else None, P(rstd.buf) if stats else None)
    for stages in ((1, 2) if split_stages else (0,)):
        assert L().clv_linear_wgrad(*args, stages, stream()) == 0
        torch.cuda.synchronize()
        if stages == 1 and (splits > 1 or stats):
            check_partials(work, splits, N, K, case, bias, what)
            eq(dw.t, case.dw0.long(), f'{what}: dW after stage 1 alone')
    eq(dw.t, case.dw, f'{what}: dW')
    eq(db.t, case.db if bias else case.db0.long(), f'{what}: db')
    for b, n in ((dy, 'dy'), (x, 'x'), (dw, 'dW'), (db, 'db'), (work, 'work')):
        b.check(f'{what}: {n}')
    if splits == 1 and not stats:
        assert torch.isnan(work.buf).all(), f'{what}: the in-place launch wrote to the work buffer'


@pytest.mark.parametrize('split_stages', [False, True], ids=['stages0', 'stages1+2'])
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('name', list(wr.SINGLE))
def test_single(name, bias, split_stages):
    c = wr.assert_single(name)
    run_single(c.M, c.N, c.K, wr.dense_case(c.M, c.N, c.K), split_stages, bias, what=name)


@pytest.mark.parametrize('M', wr.RING_M)
def test_single_ring_boundaries(M):
    """One in-place slice of M rows around the multiples of the stage (32 rows) and of the ring (4 stages): the lean loop runs
    0, 1, 2 and 3 times and the generic tail takes every length from 1 to 2 * RING - 1 stages, ragged or not."""
    N, K = wr.RING_NK
    assert L().clv_linear_wgrad_splits(M, N, K) == 1 and L().clv_linear_wgrad_in_place(M, N, K) == 1
    run_single(M, N, K, wr.dense_case(M, N, K), False, True, what=f'ring M={M} {wr.ring_trips(M)}')


@pytest.mark.parametrize('name,pad,off', [('inplace-ragged-tiles', (8, 24), (8, 16)), ('partial-one-row-tail', (16, 8), (0, 8)),
                                          ('xcd-negative-tail', (8, 8), (8, 0)), ('inplace-clamp-at-0', (24, 8), (16, 8))])
def test_single_column_slices(name, pad, off):
    """Operands that are column slices of wider tensors: ld != width, the slice starts at a multiple of 8 columns, NaN left
    and right of it."""
    c = wr.assert_single(name)
    run_single(c.M, c.N, c.K, wr.dense_case(c.M, c.N, c.K), False, True, pad, off, what=f'{name} strided')


@pytest.mark.parametrize('split_stages', [False, True], ids=['stages0', 'stages1+2'])
@pytest.mark.parametrize('name,pad', [('inplace-1000', (0, 0)), ('inplace-ragged-tiles', (8, 16)), ('partial-one-row-tail', (0, 8)),
                                      ('xcd-negative-tail', (0, 0))])
def test_standardise_on_load(name, pad, split_stages):
    """wgrad_kernel with xmean / xrstd: one slice (still partial + fold<1>) and several.  Integer means and power-of-two rstd
    make (x - mean) * rstd exact in 16 bits; rows past a slice's end must stay 0, not (0 - mean) * rstd."""
    c = wr.assert_single(name)
    run_single(c.M, c.N, c.K, wr.dense_case(c.M, c.N, c.K, stats=True), split_stages, True, pad, (0, pad[1]), what=f'{name} stats')


# ----------------------------------------------------------------------------- grouped launch
def run_group(name, flip_bias=False, seed=0, with_slots=True):
    probs = wr.GROUPS[name]
    arr = wr.assert_group(name)
    n = len(probs)
    slots = Out(SLOTS * SLOT_STRIDE, 0.0)
    keep, folds, want_ssq = [], [], 0
    for i, (e, p) in enumerate(zip(arr, probs)):
        case = wr.case_of(p, seed)
        bias = p.bias != flip_bias
        dy, x = Operand(case.dy, 8 * (i % 3), min(8 * (i % 3), 8 * (i % 2))), Operand(case.x, 8 * ((i + 1) % 3), 0)
        dw = Out(p.N * p.K, NAN if (p.in_place and p.overwrite & 1) else case.dw0)
        db = Out(p.N, case.db0)
        e.dy, e.x, e.ldy, e.ldx, e.want_bias = dy.ptr(), x.ptr(), dy.ld, x.ld, int(bias)
        work = None
        if p.in_place:
            e.dw, e.db, e.overwrite = dw.ptr(), db.ptr(), p.overwrite
            if p.overwrite & 4:
                d = case.dw_first if p.overwrite & 1 else case.dw
                want_ssq += int((d * d).sum())
        else:
            work = work_out(p.splits, p.N * p.K + p.N)
            e.work = work.ptr()
            folds.append(i)
        keep.append((case, bias, dy, x, dw, db, work))
    assert want_ssq < wr.CAP
    assert L().clv_linear_wgrad_batch_ss(arr, n, P(slots.buf) if with_slots else None, stream()) == 0
    torch.cuda.synchronize()
    for i in folds:                                            # the partial problems, before their fold
        case, bias, _, _, dw, _, work = keep[i]
        p = probs[i]
        check_partials(work, p.splits, p.N, p.K, case, bias, f'{name}[{i}]')
        eq(dw.t, case.dw0.long(), f'{name}[{i}]: dW before the fold')
    if folds:
        ent = (_lib.ClvFoldEntry * len(folds))()
        for f, i in zip(ent, folds):
            case, bias, _, _, dw, db, work = keep[i]
            p = probs[i]
            f.partial, f.dw, f.db = work.ptr(), dw.ptr(), (db.ptr() if bias else None)
            f.nk, f.e2, f.splits, f.overwrite = p.N * p.K, p.N * p.K + p.N, p.splits, 0
        assert L().clv_wgrad_fold_batch_ss(ent, len(folds), P(slots.buf) if with_slots else None, stream()) == 0
        torch.cuda.synchronize()
    for i, (p, (case, bias, dy, x, dw, db, work)) in enumerate(zip(probs, keep)):
        what = f'{name}[{i}] {p.M}x{p.N}x{p.K} cls {p.cls} {"in place" if p.in_place else "partial"} ow {p.overwrite}'
        eq(dw.t, case.dw_first if (p.in_place and p.overwrite & 1) else case.dw, what + ': dW')
        eq(db.t, case.db if bias else case.db0.long(), what + ': db')
        for b in (dy, x, dw, db) + ((work,) if work else ()):
            b.check(what)
    # WHICH of the 64 slots a workgroup adds to (its block index modulo 64) is deliberately not pinned: it is a contention
    # measure with no meaning to the consumer, which adds all slots up.  Checked: the exact total, and that nothing lands
    # in the 15 floats between two slots or past the last one.
    s = slots.t.cpu()
    per_slot = s.view(SLOTS, SLOT_STRIDE)
    assert torch.equal(per_slot[:, 1:], torch.zeros(SLOTS, SLOT_STRIDE - 1)), f'{name}: floats between the norm slots written'
    slots.check(f'{name}: norm slots')
    got = per_slot[:, 0].double().sum().item()
    assert got == (want_ssq if with_slots else 0), f'{name}: norm slots sum to {got}, the exact sum of squares is {want_ssq}'
    return want_ssq


@pytest.mark.parametrize('flip_bias', [False, True], ids=['bias-as-listed', 'bias-flipped'])
@pytest.mark.parametrize('name', ['mixed', 'twenty', 'big-alone', 'slots'])
def test_group(name, flip_bias):
    """One clv_linear_wgrad_batch_ss call (+ the batched fold of its partial problems), issued twice on fresh buffers: nothing
    may be left in tables, rings or slots.  Launches without a bit-2 entry must leave the zeroed norm slots untouched."""
    for rep in range(2):
        ssq = run_group(name, flip_bias)
        assert (ssq > 0) == any(p.overwrite & 4 for p in wr.GROUPS[name])


def test_group_without_slot_buffer():
    """bit 2 with a null slot pointer: the entry is still stored / accumulated, no sum is delivered anywhere"""
    run_group('slots', with_slots=False)


# ----------------------------------------------------------------------------- folds from synthetic partials
def fold_buffers(f, flags, sparse=False, seed=0):
    partial, dw0, db0 = wr.fold_case(f.splits, f.N, f.K, seed, sparse)
    E2 = f.N * f.K + f.N
    work = Out(f.splits * E2, partial, tail=4096)
    dw = Out(f.N * f.K, NAN if flags & 1 else dw0)
    db = Out(f.N, NAN if (flags & 2 and f.with_db) else db0)
    ref = wr.fold_exact_ref(partial, f.N, f.K, dw0, db0, bool(flags & 1), bool(flags & 2))
    if not f.with_db:
        ref = (ref[0], db0.long())
    return work, dw, db, ref


def check_fold(f, work, dw, db, ref, what):
    eq(dw.t, ref[0], f'{what}: dW')
    eq(db.t, ref[1], f'{what}: db')
    for b in (work, dw, db):
        b.check(what)


FOLD_IDS = [f'{f.splits}x{f.N}x{f.K}-{"db" if f.with_db else "nodb"}-sg{f.sg}' for f in wr.FOLDS]


@pytest.mark.parametrize('f', [f for f in wr.FOLDS if f.M], ids=[i for i, f in zip(FOLD_IDS, wr.FOLDS) if f.M])
def test_fold_stage2(f):
    """clv_linear_wgrad(stages = 2) alone on integer partials: fold_partials_kernel<1>, <4> and <16>.  (One slice folds only
    on the standardise-on-load route, so that case passes statistics; stage 2 does not read them.)"""
    wr.assert_fold(f)
    work, dw, db, ref = fold_buffers(f, 0)
    dummy = torch.zeros(8, device=DEV)
    st = P(dummy) if f.splits == 1 else None
    assert (L().clv_linear_wgrad_in_place(f.M, f.N, f.K) == 1) == (f.splits == 1)
    rc = L().clv_linear_wgrad(P(dummy), P(dummy), P(dw.buf), P(db.buf) if f.with_db else None, P(work.buf), f.M, f.N, f.K,
                              f.N, f.K, st, st, 2, stream())
    torch.cuda.synchronize()
    assert rc == 0
    check_fold(f, work, dw, db, ref, f'stage 2 {f}')


@pytest.mark.parametrize('flags', [0, 1, 2, 3])
@pytest.mark.parametrize('f', wr.FOLDS, ids=FOLD_IDS)
def test_fold_batch_one_entry(f, flags):
    """fold_batch_kernel, one entry: overwrite bit 0 against a NaN dW and bit 1 against a NaN db (stored, never read)."""
    if flags & 2 and not f.with_db:
        flags &= 1                                             # no db: bit 1 has nothing to act on, the NaN-free db stays
    wr.assert_fold(f)
    work, dw, db, ref = fold_buffers(f, flags)
    ent = (_lib.ClvFoldEntry * 1)()
    e = ent[0]
    e.partial, e.dw, e.db = work.ptr(), dw.ptr(), (db.ptr() if f.with_db else None)
    e.nk, e.e2, e.splits, e.overwrite = f.N * f.K, f.N * f.K + f.N, f.splits, flags
    e.sg_shift, e.block_begin = 7, 12345                       # the callee's to fill in (on its copy): garbage must not matter
    slots = Out(SLOTS * SLOT_STRIDE, 0.0)
    assert L().clv_wgrad_fold_batch_ss(ent, 1, P(slots.buf), stream()) == 0
    torch.cuda.synchronize()
    check_fold(f, work, dw, db, ref, f'batched fold {f} flags {flags}')
    assert not slots.t.any(), 'a fold without bit 2 wrote to the norm slots'
    slots.check('slots')


@pytest.mark.parametrize('with_slots', [True, False], ids=['slots', 'noslots'])
def test_fold_batch_many_entries(with_slots):
    """Entries with 1, 4 and 16 slice-lanes and every overwrite bit in ONE launch, twice; the entries with bit 2 deliver the
    exact sum of squares of the dW they leave behind, the others nothing."""
    for rep in range(2):
        n = len(wr.FOLD_LAUNCH)
        ent = (_lib.ClvFoldEntry * n)()
        keep, want = [], 0
        for e, (f, flags) in zip(ent, wr.FOLD_LAUNCH):
            wr.assert_fold(f)
            work, dw, db, ref = fold_buffers(f, flags, sparse=True, seed=rep)
            e.partial, e.dw, e.db = work.ptr(), dw.ptr(), (db.ptr() if f.with_db else None)
            e.nk, e.e2, e.splits, e.overwrite = f.N * f.K, f.N * f.K + f.N, f.splits, flags
            if flags & 4:
                want += int((ref[0] * ref[0]).sum())
            keep.append((f, flags, work, dw, db, ref))
        assert {f.sg for f, _ in wr.FOLD_LAUNCH} == {1, 4, 16} and 0 < want < wr.CAP
        slots = Out(SLOTS * SLOT_STRIDE, 0.0)
        assert L().clv_wgrad_fold_batch_ss(ent, n, P(slots.buf) if with_slots else None, stream()) == 0
        torch.cuda.synchronize()
        for f, flags, work, dw, db, ref in keep:
            check_fold(f, work, dw, db, ref, f'batched fold of many, {f} flags {flags}')
        per_slot = slots.t.cpu().view(SLOTS, SLOT_STRIDE)
        assert not per_slot[:, 1:].any()
        got = per_slot[:, 0].double().sum().item()
        assert got == (want if with_slots else 0), f'norm slots sum to {got}, the exact sum of squares is {want}'
        slots.check('slots')


# ----------------------------------------------------------------------------- clv_colsum
@pytest.mark.parametrize('pad', [0, 24], ids=['dense', 'strided'])
@pytest.mark.parametrize('N', wr.COLSUM_N)
@pytest.mark.parametrize('M', wr.COLSUM_M)
def test_colsum(M, N, pad):
    case = wr.dense_case(M, N, 8)
    dy = Operand(case.dy, pad, pad and 8)
    db = Out(N, case.db0)
    assert L().clv_colsum(C.c_void_p(dy.ptr()), P(db.buf), M, N, dy.ld, stream()) == 0
    torch.cuda.synchronize()
    eq(db.t, case.db, f'colsum {M}x{N} ld {dy.ld}')
    dy.check('colsum')
    db.check('colsum db')


# ----------------------------------------------------------------------------- host chunking through ops.defer_folds()
def _ops_items(shapes, shared):
    """-> [(case, dy, x, dw Out, db Out)]; problems listed in `shared` write the dW / db of problem 0"""
    items = []
    for i, (M, N, K) in enumerate(shapes):
        case = wr.dense_case(M, N, K, seed=i)
        dy, x = Operand(case.dy), Operand(case.x)
        if i in shared:
            dw, db = items[0][3], items[0][4]
        else:
            dw, db = Out(N * K, case.dw0), Out(N, case.db0)
        items.append((case, dy, x, dw, db))
    return items


@pytest.mark.parametrize('name', list(wr.OPS))
def test_ops_deferred_chunking(name, monkeypatch):
    """The planning facts of every launch the host will cut (wr.assert_ops), then the cut itself: the grouped launches as
    ops.wgrad_chunks sees the queued items, and the FoldItems the segment REALLY hands to ops.flush_folds at its end (their
    slice counts, and how ops.fold_chunks splits them), recorded on the way to the real flush."""
    from clover_amd import ops
    c = wr.assert_ops(name)
    shared = set(c.shared)
    items = _ops_items([(p.M, p.N, p.K) for p in c.probs], shared)
    sink = lambda o, shape: o.t.view(shape)
    seen = []
    real_flush = ops.flush_folds

    def recording_flush(pending):
        seen.append(([it.splits for it in pending], [len(ch) for ch in ops.fold_chunks(pending)]))
        return real_flush(pending)

    monkeypatch.setattr(ops, 'flush_folds', recording_flush)
    with ops.defer_folds() as seg:
        for case, dy, x, dw, db in items:
            N, K = case.dw0.shape
            assert ops.linear_wgrad(dy.view, x.view, True, sink(dw, (N, K)), sink(db, (N,))) == (None, None)
        assert seg.wgrads is not None and len(seg.wgrads) == len(items) and not seg.folds
        assert [len(ch) for ch in ops.wgrad_chunks(seg.wgrads)] == list(c.launches)
    assert seen == [(list(c.fold_splits), list(c.fold_launches))], f'{name}: the segment folded {seen}'
    torch.cuda.synchronize()
    for i, (case, dy, x, dw, db) in enumerate(items):
        if i in shared:
            continue
        users = [j for j in shared | {0}] if (i == 0 and shared) else [i]
        ref_w = case.dw0.long() + sum(items[j][0].dw_first for j in users)
        ref_b = case.db0.long() + sum(items[j][0].db - items[j][0].db0.long() for j in users)
        eq(dw.t, ref_w, f'ops problem {i}: dW')
        eq(db.t, ref_b, f'ops problem {i}: db')
        dw.check(f'ops problem {i}')
        db.check(f'ops problem {i}')


# ----------------------------------------------------------------------------- random data: two bounds, neither fitted
def hold(what, M, splits, got_w, got_b, ref):
    """Per tensor: max|err| / max|ref| <= F32_BOUND.  Per element: |err| <= (M + splits + 2) * 2^-23 * absdot, the standard
    bound of a sum of M products plus `splits` partials plus the accumulate, for ANY order of accumulation; deliberately
    loose (the integer cases catch structure, this one a precision regression such as a 16-bit intermediate)."""
    dw, db, absdot, absdot_b = ref
    bad = []
    for name, g, r, a in (('dW', got_w, dw, absdot), ('db', got_b, db, absdot_b)):
        if g is None:
            continue
        g = g.detach().cpu().double().reshape(r.shape)
        assert torch.isfinite(g).all(), f'{what} {name}: non-finite values'
        err = (g - r).abs()
        tens = (err.max() / r.abs().max()).item()
        elem = (err / ((M + splits + 2) * U * a).clamp_min(1e-300)).max().item()
        print(f'WGRAD_BUDGET | {what} | {name} | max/max {tens:.2e} = {tens / F32_BOUND:.3f} of the bound | '
              f'per element {elem:.2e} of the bound')
        if tens > F32_BOUND:
            bad.append(f'{name}: max error {tens:.3e} of the maximum (allowed {F32_BOUND})')
        if elem > 1:
            bad.append(f'{name}: an element is off by {elem:.3f} x its summation bound')
    assert not bad, f'{what}: ' + '; '.join(bad)


@pytest.mark.parametrize('name', ['xcd-negative-tail', 'inplace-1000'])
def test_random_data_single(name):
    c = wr.assert_single(name)
    dy_, x_, dw0, db0 = wr.gauss_case(c.M, c.N, c.K)
    dy, x, dw, db = Operand(dy_), Operand(x_), Out(c.N * c.K, dw0), Out(c.N, db0)
    work = work_out(c.splits, c.N * c.K + c.N)
    assert L().clv_linear_wgrad(C.c_void_p(dy.ptr()), C.c_void_p(x.ptr()), P(dw.buf), P(db.buf), P(work.buf), c.M, c.N, c.K,
                                dy.ld, x.ld, None, None, 0, stream()) == 0
    torch.cuda.synchronize()
    kind = 'in place' if c.splits == 1 else 'partial + fold'
    hold(f'stand-alone {kind} {c.M}x{c.N}x{c.K} ({c.splits} slices)', c.M, c.splits, dw.t, db.t, wr.f64_ref(dy_, x_, dw0, db0))
    for b in (dw, db, work):
        b.check(name)


@pytest.mark.parametrize('name', ['small-alone', 'big-alone'])
def test_random_data_group(name):
    (p,) = wr.GROUPS[name]
    arr = wr.assert_group(name)
    dy_, x_, dw0, db0 = wr.gauss_case(p.M, p.N, p.K)
    dy, x, dw, db = Operand(dy_), Operand(x_), Out(p.N * p.K, dw0), Out(p.N, db0)
    work = work_out(p.splits, p.N * p.K + p.N)
    e = arr[0]
    e.dy, e.x, e.ldy, e.ldx, e.want_bias, e.work = dy.ptr(), x.ptr(), dy.ld, x.ld, 1, work.ptr()
    assert L().clv_linear_wgrad_batch_ss(arr, 1, None, stream()) == 0
    ent = (_lib.ClvFoldEntry * 1)()
    f = ent[0]
    f.partial, f.dw, f.db, f.nk, f.e2, f.splits = work.ptr(), dw.ptr(), db.ptr(), p.N * p.K, p.N * p.K + p.N, p.splits
    assert L().clv_wgrad_fold_batch_ss(ent, 1, None, stream()) == 0
    torch.cuda.synchronize()
    hold(f'grouped {128 * (1 + p.cls)}-class {p.M}x{p.N}x{p.K} ({p.splits} slices) + batched fold', p.M, p.splits, dw.t, db.t,
         wr.f64_ref(dy_, x_, dw0, db0))
    for b in (dw, db, work):
        b.check(name)


def test_random_data_fold():
    f = wr.Fold(33, 136, 72, True, 16)
    wr.assert_fold(f)
    g = torch.Generator().manual_seed(5)
    E2 = f.N * f.K + f.N
    partial, dw0, db0 = torch.randn(f.splits, E2, generator=g), torch.randn(f.N, f.K, generator=g), torch.randn(f.N, generator=g)
    work, dw, db = Out(f.splits * E2, partial), Out(f.N * f.K, dw0), Out(f.N, db0)
    ent = (_lib.ClvFoldEntry * 1)()
    e = ent[0]
    e.partial, e.dw, e.db, e.nk, e.e2, e.splits = work.ptr(), dw.ptr(), db.ptr(), f.N * f.K, E2, f.splits
    assert L().clv_wgrad_fold_batch_ss(ent, 1, None, stream()) == 0
    torch.cuda.synchronize()
    s, a = partial.double().sum(0), partial.double().abs().sum(0)
    NK = f.N * f.K
    ref = (s[:NK].reshape(f.N, f.K) + dw0.double(), s[NK:] + db0.double(), a[:NK].reshape(f.N, f.K) + dw0.double().abs(),
           a[NK:] + db0.double().abs())
    hold(f'batched fold {f.splits}x{f.N}x{f.K} ({f.sg} lanes)', 0, f.splits, dw.t, db.t, ref)
