"""References, input generators and planning claims for the weight-gradient tests (tests/test_wgrad_ref_cpu.py,
tests/test_wgrad_gpu.py).  Plain torch on the CPU; the only library calls are the HOST planning entries.

    dW[n][k] = (0 if first else dw0[n][k]) + sum_m dy[m][n] x[m][k]          db[n] = db0[n] + sum_m dy[m][n]

Exactness.  The generators produce INTEGER-valued 16-bit operands and integer-valued fp32 accumulators, and assert on the
reference  max(|dw0| + |dy|^T |x|) < 2^24  (and the same for db).  Every partial sum of such a dot product, in any order and
any grouping (MFMA blocks, M-slices, fold lanes), is then an integer below 2^24 in magnitude: exactly representable in fp32,
so every fp32 addition is exact and the kernel's result must equal the int64 reference bit for bit (torch.equal).  The
norm-slot cases additionally assert  sum dW_final^2 < 2^24, which makes the kernels' sums of squares exact in the same way.
These are caps on the INPUTS, checked on the reference; they are not tolerances.

Claims.  Slice counts, work sizes, tile class and in-place-or-not come from the library's host entries and are compared with
literals below.  Three facts have no host entry and are hand-written COPIES of conditions in csrc/gemm_wgrad.hip, so a retune
of those conditions moves cases quietly instead of failing a claim: fold_sg() (the lane thresholds of stage 2 and of
clv_wgrad_fold_batch_ss, which fills sg_shift on a copy of the table), the `xcd` flag of single_plan() (xcd_map of
clv_linear_wgrad) and ring_trips() (the lean-loop condition).  Whoever edits those lines edits these.
"""
import functools
from typing import NamedTuple, Optional, Tuple

import torch

from clover_amd import _lib

HALF = _lib.half_dtype()
CAP = 1 << 24
# the kernels' own constants the claims below are stated in (csrc/gemm_wgrad.hip: TM, SM, WG_RING); a change of one of them
# moves the ring-boundary cases off their paths and must be followed here
TM, SM, RING = 64, 32, 4


# ----------------------------------------------------------------------------------------------- references
def _i64(t):
    d = t.double()
    assert torch.equal(d, d.round()), 'the exact reference takes integer-valued inputs only'
    return d.to(torch.int64)


def exact_ref(dy, x, dw0, db0, first=False):
    """int64 (dW, db).  dw0 / db0 may be None (= 0); `first`: dW is stored, dw0 is never read (it may hold NaN)."""
    dy, x = _i64(dy), _i64(x)
    dw = dy.t().contiguous() @ x
    if not first and dw0 is not None:
        dw = dw + _i64(dw0)
    db = dy.sum(0)
    if db0 is not None:
        db = db + _i64(db0)
    return dw, db


def f64_ref(dy, x, dw0, db0, first=False):
    """fp64 (dW, db, absdot, absdot_b): absdot = |dw0| + |dy|^T |x| per element of dW, absdot_b = |db0| + sum |dy|."""
    dy, x = dy.double(), x.double()
    dw = dy.t() @ x
    absdot = dy.abs().t() @ x.abs()
    if not first and dw0 is not None:
        dw = dw + dw0.double()
        absdot = absdot + dw0.double().abs()
    db, absdot_b = dy.sum(0), dy.abs().sum(0)
    if db0 is not None:
        db, absdot_b = db + db0.double(), absdot_b + db0.double().abs()
    return dw, db, absdot, absdot_b


def fold_exact_ref(partial, N, K, dw0, db0, store_dw=False, store_db=False):
    """int64 (dW, db) of a fold of partial [splits][N*K + N] into dw0 / db0 (store_*: the target is not read)."""
    s = _i64(partial).sum(0)
    dw, db = s[:N * K].reshape(N, K), s[N * K:]
    if not store_dw:
        dw = dw + _i64(dw0)
    if not store_db and db0 is not None:
        db = db + _i64(db0)
    return dw, db


# ----------------------------------------------------------------------------------------------- generators
class Case(NamedTuple):
    dy: torch.Tensor            # HALF [M][N], integer-valued
    x: torch.Tensor             # HALF [M][K], integer-valued (the raw operand; with stats: before standardisation)
    dw0: torch.Tensor           # fp32 [N][K], integer-valued: what dW holds before the launch
    db0: torch.Tensor           # fp32 [N]
    dw: torch.Tensor            # int64 reference, accumulated (dw0 + dy^T x)
    db: torch.Tensor            # int64 reference (db0 + colsum dy)
    dw_first: torch.Tensor      # int64 reference, stored (dy^T x)
    mean: Optional[torch.Tensor] = None     # fp32 [M]: standardise-on-load statistics (integer means, power-of-two rstd)
    rstd: Optional[torch.Tensor] = None


def _check_caps(dy, x, dw0, db0):
    absdot = (dy.double().abs().t() @ x.double().abs() + dw0.double().abs()).max().item()
    assert absdot < CAP, f'|dw0| + |dy|^T|x| reaches {absdot} >= 2^24: fp32 accumulation would depend on the order'
    absb = (dy.double().abs().sum(0) + db0.double().abs()).max().item()
    assert absb < CAP, f'|db0| + sum|dy| reaches {absb} >= 2^24'
    for t in (dy, x):
        assert torch.equal(t.double(), t.double().round()) and t.dtype == HALF


def _finish(dy, x, dw0, db0, norm, xop=None, mean=None, rstd=None):
    xop = x if xop is None else xop
    _check_caps(dy, xop, dw0, db0)
    dw, db = exact_ref(dy, xop, dw0, db0)
    dw_first, _ = exact_ref(dy, xop, None, None, first=True)
    if norm:
        for name, t in (('accumulated', dw), ('stored', dw_first)):
            q = int((t * t).sum())
            assert q < CAP, f'sum of squares of the {name} dW is {q} >= 2^24: the norm slots would not be exact'
    return Case(dy, x, dw0, db0, dw, db, dw_first, mean, rstd)


@functools.lru_cache(maxsize=None)
def dense_case(M, N, K, seed=0, stats=False):
    """Operands in [-3, 3], accumulators in [-8, 8].  stats: per-row integer means in [-2, 2] and rstd in {1, 2, 4}; the
    reference then uses (x - mean) * rstd, an integer of magnitude <= 20: exact in bf16 and fp16, so the kernel's 16-bit
    rounding of the standardised operand is the identity."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)
    dy, x = ri(-3, 3, M, N).to(HALF), ri(-3, 3, M, K).to(HALF)
    dw0, db0 = ri(-8, 8, N, K).float(), ri(-8, 8, N).float()
    if not stats:
        return _finish(dy, x, dw0, db0, False)
    mean = ri(-2, 2, M).float()
    rstd = torch.tensor([1.0, 2.0, 4.0])[ri(0, 2, M)]
    xhat = (x.float() - mean[:, None]) * rstd[:, None]
    assert torch.equal(xhat.to(HALF).float(), xhat)
    return _finish(dy, x, dw0, db0, False, xop=xhat.to(HALF), mean=mean, rstd=rstd)


@functools.lru_cache(maxsize=None)
def sparse_case(M, N, K, seed=0):
    """Operands in {-1, 0, 1} with the density p that puts E[sum dW^2] = N K M p^2 at 2^21, dw0 in {-1, 0, 1} with at most
    ~2^19 non-zeros: sum (dw0 + dy^T x)^2 <= 2 (2^19 + 2^21) in expectation, an eighth of the way to 2^24 — asserted on
    the reference, not assumed."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K + 1)
    p = min(1.0, ((1 << 21) / (N * K * M)) ** 0.5)
    p0 = min(1.0, (1 << 19) / (N * K))

    def tern(dens, *shape):
        keep = torch.rand(shape, generator=g) < dens
        return (torch.randint(0, 2, shape, generator=g) * 2 - 1) * keep

    dy, x = tern(p, M, N).to(HALF), tern(p, M, K).to(HALF)
    dw0, db0 = tern(p0, N, K).float(), torch.randint(-8, 9, (N,), generator=g).float()
    return _finish(dy, x, dw0, db0, True)


@functools.lru_cache(maxsize=None)
def fold_case(splits, N, K, seed=0, sparse=False):
    """Synthetic integer partials [splits][N*K + N] in [-4, 4] (sparse: {-1, 0, 1}, so that sum dW_final^2 < 2^24) with
    integer targets -> (partial fp32, dw0, db0)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * splits + 31 * N + K + 2)
    E2 = N * K + N
    if sparse:
        dens = min(1.0, (1 << 20) / (N * K * splits))
        partial = ((torch.randint(0, 2, (splits, E2), generator=g) * 2 - 1) * (torch.rand(splits, E2, generator=g) < dens)).float()
        dw0 = ((torch.randint(0, 2, (N, K), generator=g) * 2 - 1) * (torch.rand(N, K, generator=g) < min(1.0, (1 << 19) / (N * K)))).float()
    else:
        partial = torch.randint(-4, 5, (splits, E2), generator=g).float()
        dw0 = torch.randint(-8, 9, (N, K), generator=g).float()
    db0 = torch.randint(-8, 9, (N,), generator=g).float()
    top = (partial.double().abs().sum(0).max() + 8).item()
    assert top < CAP
    if sparse:
        for store in (False, True):
            dw, _ = fold_exact_ref(partial, N, K, dw0, db0, store_dw=store)
            assert int((dw * dw).sum()) < CAP
    return partial, dw0, db0


@functools.lru_cache(maxsize=None)
def gauss_case(M, N, K, seed=0):
    """Gaussian 16-bit operands and fp32 accumulators for the random-data bound -> (dy, x, dw0, db0)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K + 3)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(M, N).to(HALF), r(M, K).to(HALF), r(N, K) * M ** 0.5, r(N) * M ** 0.5


# ----------------------------------------------------------------------------------------------- planning claims
def roundup(v, to):
    return (v + to - 1) // to * to


def slice_rows(M, splits):
    """rows_per_split of clv_linear_wgrad / clv_linear_wgrad_batch_ss, and m_end - m_begin of every slice (the host rounds
    the slice length up to TM AFTER fixing the slice count, so the last ones may be empty or start past M: negative)."""
    rows = roundup(-(-M // splits), TM)
    return rows, [min(M, (s + 1) * rows) - s * rows for s in range(splits)]


def ring_trips(rows):
    """(trips of the lean 4-stage loop, stages left to the generic tail) of one slice of `rows` rows: the prologue issues
    RING - 1 stages, the lean loop runs while issued + RING <= complete stages."""
    if rows <= 0:
        return 0, 0
    nst, nfull = -(-rows // SM), rows // SM
    trips = max(0, (nfull - (RING - 1)) // RING)
    return trips, nst - trips * RING


def fold_sg(N, K, splits, with_db):
    """Slice-lanes per element group of the fold kernels (the thresholds of clv_linear_wgrad stage 2 and of
    clv_wgrad_fold_batch_ss; the callee works on a copy of the entry table, so sg_shift is not visible from outside)."""
    groups = (N * K + (N if with_db else 0) + 3) // 4
    return 1 if (groups >= (1 << 17) or splits < 8) else 4 if (groups >= (1 << 15) or splits < 32) else 16


class Single(NamedTuple):       # one stand-alone clv_linear_wgrad problem and what the planner must say about it
    M: int
    N: int
    K: int
    splits: int
    rows: int                   # rows_per_split
    tail: Tuple[int, ...]       # row counts of the last slices (as many as listed)
    xcd: bool                   # XCD-mapped block order (splits >= 8 and tiles >= 4)


# name -> claim.  In place <=> splits == 1.
SINGLE = {
    'inplace-ragged-tiles': Single(40, 480, 672, 1, 64, (40,), False),
    'inplace-clamp-at-0': Single(33, 8, 8, 1, 64, (33,), False),
    'inplace-1000': Single(1000, 136, 72, 1, 1024, (1000,), False),
    'partial-one-row-tail': Single(1025, 136, 72, 5, 256, (256, 1), False),
    'partial-one-row-tail-9': Single(2049, 96, 96, 9, 256, (256, 1), False),
    'xcd-empty-tail': Single(4800, 512, 512, 16, 320, (320, 0), True),
    'xcd-negative-tail': Single(4700, 512, 512, 16, 320, (220, -100), True),
    'xcd-padding-blocks': Single(2500, 256, 512, 10, 256, (256, 196), True),     # 10 slices on 16 XCD slots
    # 33 slices, the last of 8 rows: the stand-alone fold with 16 lanes and a ragged slice count (3, 2, 2, ... per lane)
    'partial-33-slices': Single(8200, 136, 72, 33, 256, (256, 8), False),
}
# ring boundaries, in place (one slice of M rows): lean loop 0 times with every tail length 1 .. 7, then once and twice
RING_M = (1, 31, 32, 33, 64, 96, 97, 128, 129, 160, 192, 223, 224, 225, 256, 288, 320, 351, 352, 353, 480, 481)
RING_NK = (136, 72)


def single_plan(M, N, K):
    """What the library's host entries say about a stand-alone problem, in the shape of a Single."""
    L = _lib.lib()
    splits = L.clv_linear_wgrad_splits(M, N, K)
    assert L.clv_linear_wgrad_work_floats(M, N, K) == splits * (N * K + N)
    rows, sl = slice_rows(M, splits)
    tiles = -(-N // 128) * -(-K // 128)
    return splits, rows, sl, splits >= 8 and tiles >= 4


def assert_single(name):
    c = SINGLE[name]
    splits, rows, sl, xcd = single_plan(c.M, c.N, c.K)
    got = Single(c.M, c.N, c.K, splits, rows, tuple(sl[-len(c.tail):]), xcd)
    assert got == c, f'{name}: the planner moved this case off its path: {got} (claimed {c})'
    return c


class Prob(NamedTuple):         # one problem of a grouped launch and what clv_linear_wgrad_batch_plan must say about it
    M: int
    N: int
    K: int
    cls: int                    # 0: 128 x 128 tiles, 1: 256 x 256 tiles
    in_place: bool
    splits: int
    rows: int
    tail: Tuple[int, ...]
    bias: bool = True
    overwrite: int = 0          # in-place entries: bit 0 store dW, bit 2 norm slots
    sparse: bool = False        # sparse generator (norm-slot entries and whatever shares their launch's slots)


_TINY = tuple(Prob(33 + 7 * i, 8, 8 + 8 * (i % 3), 0, True, 1, roundup(33 + 7 * i, TM), (33 + 7 * i,), bias=bool(i & 1))
              for i in range(15))
GROUPS = {
    # every kind of problem in one call: 128-class partial / in place, 256-class partial / in place
    'mixed': (Prob(1281, 96, 288, 0, False, 6, 256, (256, 1)),
              Prob(40, 480, 672, 0, True, 1, 64, (40,), overwrite=1),
              Prob(33, 8, 8, 0, True, 1, 64, (33,), bias=False),
              Prob(4700, 512, 512, 1, False, 12, 448, (220, -228), bias=False),
              Prob(1100, 1024, 1280, 1, True, 1, 1152, (1100,), overwrite=5, sparse=True)),
    # 20 problems of the 128 class: the per-problem target drops to 102 workgroups and the 6-tile problem gets 17 slices
    'twenty': (Prob(4700, 264, 136, 0, False, 17, 320, (220, -100, -420)),
               Prob(1025, 8, 8, 0, False, 5, 256, (256, 1)),
               Prob(1100, 16, 8, 0, False, 5, 256, (256, 76), bias=False),
               Prob(2049, 8, 24, 0, False, 9, 256, (256, 1)),
               Prob(40, 136, 72, 0, True, 1, 64, (40,), overwrite=1, bias=False)) + _TINY,
    'big-alone': (Prob(4700, 512, 512, 1, False, 12, 448, (220, -228)),),
    'small-alone': (Prob(4700, 264, 136, 0, False, 19, 256, (256, 92)),),
    # norm slots: every in-place entry carries bit 2 (one stores, one accumulates), sparse data throughout
    'slots': (Prob(1100, 1024, 1280, 1, True, 1, 1152, (1100,), overwrite=5, sparse=True),
              Prob(40, 480, 672, 0, True, 1, 64, (40,), overwrite=4, sparse=True),
              Prob(1000, 136, 72, 0, True, 1, 1024, (1000,), overwrite=5, sparse=True, bias=False),
              Prob(1281, 96, 288, 0, False, 6, 256, (256, 1), sparse=True)),
}


def group_plan(probs):
    """clv_linear_wgrad_batch_plan on the launch's shapes -> the planned ClvWgradEntry array."""
    L = _lib.lib()
    arr = (_lib.ClvWgradEntry * len(probs))()
    for e, p in zip(arr, probs):
        e.M, e.N, e.K = p.M, p.N, p.K
    assert L.clv_linear_wgrad_batch_plan(arr, len(probs)) == 0
    return arr


def assert_group(name, probs=None):
    """The planning facts of every problem of GROUPS[name] (or of `probs`, one launch) through the library's entries -> the
    planned entries."""
    L = _lib.lib()
    probs = GROUPS[name] if probs is None else probs
    arr = group_plan(probs)
    for i, (e, p) in enumerate(zip(arr, probs)):
        rows, sl = slice_rows(p.M, e.splits)
        got = (L.clv_linear_wgrad_class(p.M, p.N, p.K), bool(L.clv_linear_wgrad_in_place(p.M, p.N, p.K)), e.splits, rows,
               tuple(sl[-len(p.tail):]))
        assert got == (p.cls, p.in_place, p.splits, p.rows, p.tail), \
            f'{name}[{i}] {p.M}x{p.N}x{p.K}: the planner moved this problem off its path: {got} (claimed {p[3:8]})'
        assert e.work_floats == (0 if p.in_place else p.splits * (p.N * p.K + p.N))
    return arr


class OpsCase(NamedTuple):      # problems queued inside ops.defer_folds(), in order, and how the host must cut them up
    probs: Tuple[Prob, ...]     # claims per problem, as planned inside ITS launch
    shared: frozenset           # indices of the problems that write the dW / db of problem 0
    launches: Tuple[int, ...]   # problems per grouped launch
    fold_launches: Tuple[int, ...]      # entries per batched fold launch
    fold_splits: Tuple[int, ...]        # slice counts of the FoldItems the segment produces, in order


_IP = lambda M, N, K: Prob(M, N, K, 0, True, 1, roundup(M, TM), (M,))
OPS = {
    # two in-place uses of one dW never share a launch (no atomics): [A] then [A', tiny]
    'shared-in-place': OpsCase((_IP(40, 480, 672), _IP(40, 480, 672), _IP(33, 8, 8)), frozenset({1}), (1, 2), (), ()),
    # two partial uses of one dW: one launch (3 problems of class 0: 5 slices each, last of 1 row), their folds one by one
    'shared-partial': OpsCase((Prob(1025, 136, 72, 0, False, 5, 256, (256, 1)), Prob(1025, 136, 72, 0, False, 5, 256, (256, 1)),
                               _IP(33, 8, 8)), frozenset({1}), (3,), (1, 1), (5, 5)),
    'more-than-a-launch': OpsCase(tuple(_IP(33 + i, 8, 8) for i in range(_lib.WGRAD_GROUP_MAX + 5)), frozenset(),
                                  (_lib.WGRAD_GROUP_MAX, 5), (), ()),
}


def assert_ops(name):
    """Every launch of OPS[name] planned on its own, as the host chunker will issue it."""
    c = OPS[name]
    assert sum(c.launches) == len(c.probs)
    at = 0
    for n in c.launches:
        assert_group(f'{name} launch at {at}', c.probs[at:at + n])
        at += n
    return c


class Fold(NamedTuple):         # a fold from synthetic partials: shape, whether db is folded, and the slice-lanes it runs with
    splits: int
    N: int
    K: int
    with_db: bool
    sg: int
    M: int = 0                  # an M for which the stand-alone planner picks `splits` slices (0: batched entry only)


def _fold_m(splits):
    """136 x 72 is 2 tiles: the stand-alone planner picks ceil(M / 256) slices for 1024 < M (so never 2 .. 4 at this width:
    those come from outputs of >= 64 tiles, see the 1024 x 1024 entry), one for M <= 1024 (folded only with statistics);
    33 slices at M = 8200 exactly (ceil(8200 / 256) = 33), the largest M of these tests; 67 would need M > 8200 and runs
    through the batched entry only."""
    return 156 if splits == 1 else 8200 if splits == 33 else 256 * splits - 100 if 5 <= splits <= 32 else 0


FOLDS = tuple(Fold(s, 136, 72, db, 1 if s < 8 else 4 if s < 32 else 16, _fold_m(s))
              for s in (1, 3, 4, 7, 8, 31, 32, 33, 67) for db in (True, False)) + (
    # both sides of 2^15 element groups (>= 32 slices: 16 lanes below, 4 from there) and of 2^17 (4 below, 1 from there)
    Fold(32, 128, 1016, False, 16, 8100), Fold(32, 128, 1024, False, 4, 8100),
    Fold(33, 128, 1016, True, 16), Fold(33, 128, 1024, True, 4),
    Fold(8, 512, 1016, False, 4, 2000), Fold(8, 512, 1024, False, 1, 2000),
    Fold(8, 512, 1016, True, 4, 2000), Fold(8, 512, 1024, True, 1, 2000),
    Fold(4, 1024, 1024, True, 1, 1100))                       # 64 tiles: 4 slices from the stand-alone planner
# one batched launch, entries of all three lane counts, every overwrite bit (0: store dW, 1: store db, 2: norm slots)
FOLD_LAUNCH = ((Fold(67, 136, 72, True, 16), 0), (Fold(3, 136, 72, True, 1), 3), (Fold(8, 136, 72, False, 4), 1),
               (Fold(33, 8, 8, True, 16), 2), (Fold(31, 96, 288, True, 4), 5), (Fold(4, 40, 24, True, 1), 4),
               (Fold(32, 136, 72, False, 16), 6))
COLSUM_M, COLSUM_N = (1, 31, 64, 65, 1000), (8, 64, 72, 200)


def assert_fold(f):
    assert fold_sg(f.N, f.K, f.splits, f.with_db) == f.sg, f'{f}: the fold would run with another lane count'
    if f.M:
        got = _lib.lib().clv_linear_wgrad_splits(f.M, f.N, f.K)
        assert got == f.splits, f'{f}: the stand-alone planner picks {got} slices for M = {f.M}'


def case_of(p, seed=0):
    return sparse_case(p.M, p.N, p.K, seed) if p.sparse else dense_case(p.M, p.N, p.K, seed)
