"""tests/wgrad_ref.py without a GPU: the int64 and the fp64 reference agree, every generator meets the caps that make fp32
accumulation order-independent at every shape tests/test_wgrad_gpu.py uses, and the planning facts those cases claim hold
through the library's own host entries (a retuned planner fails HERE, on the claim, not quietly on another path)."""
import pytest
import torch

import wgrad_ref as wr
from clover_amd import _lib


def L():
    return _lib.lib()


def _shapes():
    s = {(c.M, c.N, c.K, False) for c in wr.SINGLE.values()} | {(M,) + wr.RING_NK + (False,) for M in wr.RING_M}
    s |= {(p.M, p.N, p.K, p.sparse) for ps in wr.GROUPS.values() for p in ps}
    s |= {(M, N, 8, False) for M in wr.COLSUM_M for N in wr.COLSUM_N}
    return sorted(s)


@pytest.mark.parametrize('M,N,K,sparse', _shapes())
def test_generators_meet_their_caps_and_references_agree(M, N, K, sparse):
    """The generator asserts its caps itself (on the reference); here additionally: the values are integers of the stated
    range in the library's 16-bit type, and the fp64 reference reproduces the int64 one exactly."""
    c = wr.sparse_case(M, N, K) if sparse else wr.dense_case(M, N, K)
    top = 1 if sparse else 3
    for t in (c.dy, c.x):
        assert t.dtype == wr.HALF and t.abs().max() <= top and torch.equal(t.float(), t.float().round())
    dw, db, absdot, absdot_b = wr.f64_ref(c.dy, c.x, c.dw0, c.db0)
    assert torch.equal(dw, c.dw.double()) and torch.equal(db, c.db.double())
    assert torch.equal(wr.f64_ref(c.dy, c.x, c.dw0, c.db0, first=True)[0], c.dw_first.double())
    assert absdot.max() < wr.CAP and absdot_b.max() < wr.CAP and (absdot >= dw.abs()).all()
    if sparse:
        assert int((c.dw * c.dw).sum()) < wr.CAP and int((c.dw_first * c.dw_first).sum()) < wr.CAP
        assert int((c.dw_first * c.dw_first).sum()) > 0


@pytest.mark.parametrize('name', ['inplace-ragged-tiles', 'partial-one-row-tail', 'xcd-negative-tail'])
def test_standardised_operand_is_exact_in_16_bits(name):
    c = wr.SINGLE[name]
    case = wr.dense_case(c.M, c.N, c.K, stats=True)
    xhat = (case.x.double() - case.mean.double()[:, None]) * case.rstd.double()[:, None]
    assert torch.equal(xhat.to(wr.HALF).double(), xhat) and xhat.abs().max() <= 20
    assert set(case.rstd.tolist()) <= {1.0, 2.0, 4.0} and torch.equal(case.mean, case.mean.round())
    dw, db, _, _ = wr.f64_ref(case.dy, xhat, case.dw0, case.db0)
    assert torch.equal(dw, case.dw.double()) and torch.equal(db, case.db.double())


def test_caps_are_enforced():
    """A generator whose inputs break a cap must raise, not hand out inputs for which torch.equal proves nothing."""
    big = torch.full((4096, 8), 64.0).to(wr.HALF)
    with pytest.raises(AssertionError, match='2\\^24'):
        wr._finish(big, big, torch.zeros(8, 8), torch.zeros(8), False)
    ones = torch.ones((4096, 72)).to(wr.HALF)
    with pytest.raises(AssertionError, match='sum of squares'):
        wr._finish(ones, ones, torch.zeros(72, 72), torch.zeros(72), True)
    with pytest.raises(AssertionError, match='integer'):
        wr.exact_ref(torch.full((8, 8), 0.5), torch.ones(8, 8), None, None)


@pytest.mark.parametrize('f', wr.FOLDS + tuple(f for f, _ in wr.FOLD_LAUNCH), ids=str)
def test_fold_cases(f):
    wr.assert_fold(f)
    for sparse in (False, True):
        partial, dw0, db0 = wr.fold_case(f.splits, f.N, f.K, 0, sparse)
        assert partial.shape == (f.splits, f.N * f.K + f.N) and torch.equal(partial, partial.round())
        dw, db = wr.fold_exact_ref(partial, f.N, f.K, dw0, db0)
        s = partial.double().sum(0)
        assert torch.equal(dw.double().reshape(-1), s[:f.N * f.K] + dw0.double().reshape(-1))
        assert torch.equal(db.double(), s[f.N * f.K:] + db0.double())
        if sparse:
            assert int((dw * dw).sum()) < wr.CAP
        if f.splits * (f.N * f.K + f.N) > (1 << 20):
            break                                              # (the large ones are only used dense)
    assert f.splits * (f.N * f.K + f.N) * 4 <= 17 << 20


def test_fold_cases_reach_every_lane_count_and_both_sides_of_the_thresholds():
    assert {f.sg for f in wr.FOLDS} == {1, 4, 16} and {f.splits for f in wr.FOLDS} == {1, 3, 4, 7, 8, 31, 32, 33, 67}
    groups = lambda f: (f.N * f.K + (f.N if f.with_db else 0) + 3) // 4
    for thr, s_min, below, above in ((1 << 15, 32, 16, 4), (1 << 17, 8, 4, 1)):
        for db in (True, False):
            near = [f for f in wr.FOLDS if f.with_db == db and f.splits >= s_min and abs(groups(f) - thr) <= thr // 64]
            assert {f.sg for f in near if groups(f) < thr} == {below} and {f.sg for f in near if groups(f) >= thr} == {above}
    assert any(groups(f) == 1 << 15 for f in wr.FOLDS) and any(groups(f) == 1 << 17 for f in wr.FOLDS)


@pytest.mark.parametrize('name', list(wr.SINGLE))
def test_single_plans(name):
    c = wr.assert_single(name)
    assert (c.splits == 1) == (c.M <= 1024)                   # stand-alone: in place <=> one slice <=> few rows
    rows, sl = wr.slice_rows(c.M, c.splits)
    assert rows % wr.TM == 0 and sum(max(r, 0) for r in sl) == c.M


def test_single_plans_name_the_geometries():
    """one row, no row and a negative row count in the last slices; padding blocks of the XCD-mapped grid; both block orders"""
    tails = {n: c.tail for n, c in wr.SINGLE.items()}
    assert tails['partial-one-row-tail'][-1] == 1 and tails['partial-one-row-tail-9'][-1] == 1
    assert tails['xcd-empty-tail'][-1] == 0 and tails['xcd-negative-tail'][-1] < 0
    assert wr.SINGLE['xcd-padding-blocks'].splits % 8 != 0 and wr.SINGLE['xcd-padding-blocks'].xcd
    assert {c.xcd for c in wr.SINGLE.values() if c.splits > 1} == {True, False}
    for M in wr.RING_M:
        assert L().clv_linear_wgrad_splits(M, *wr.RING_NK) == 1


def test_ring_boundary_cases_cover_every_tail():
    """The in-place slice lengths of test_single_ring_boundaries: lean loop 0 .. 3 trips, every tail length the generic loop
    can be left with (1 .. 2 * RING - 1 stages; after a lean trip at least RING - 1), the three lengths around one ring."""
    seen = {wr.ring_trips(M) for M in wr.RING_M}
    assert {(0, t) for t in range(1, 2 * wr.RING)} <= seen and {(1, t) for t in range(wr.RING - 1, 2 * wr.RING)} <= seen
    assert {tr for tr, _ in seen} >= {0, 1, 2, 3}
    for a in (wr.SM * (wr.RING - 1), wr.SM * wr.RING, wr.SM * wr.RING + 1):
        assert a in wr.RING_M
    # the slices of the multi-slice cases: full ones run the lean loop, the last ones are ragged, one row, empty, negative
    assert wr.ring_trips(320) == (1, 6) and wr.ring_trips(448) == (2, 6) and wr.ring_trips(256) == (1, 4)
    assert wr.ring_trips(220) == (0, 7) and wr.ring_trips(1) == (0, 1) and wr.ring_trips(0) == wr.ring_trips(-100) == (0, 0)


@pytest.mark.parametrize('name', list(wr.GROUPS))
def test_group_plans(name):
    arr = wr.assert_group(name)
    assert len(arr) <= _lib.WGRAD_GROUP_MAX
    for e, p in zip(arr, wr.GROUPS[name]):
        assert not (p.overwrite and not p.in_place), 'overwrite bits act on in-place entries only'
        assert not (p.overwrite & 4) or p.sparse


def test_group_plans_name_the_geometries():
    kinds = {(p.cls, p.in_place) for p in wr.GROUPS['mixed']}
    assert kinds == {(0, False), (0, True), (1, False), (1, True)}
    assert len(wr.GROUPS['twenty']) == 20 and wr.GROUPS['twenty'][0].tail == (220, -100, -420)
    assert wr.GROUPS['big-alone'][0].tail == (220, -228)
    # the same shape gets another slice count alone: the 20-problem launch is what produces the past-the-end slices
    assert wr.group_plan([wr.GROUPS['twenty'][0]])[0].splits == wr.GROUPS['small-alone'][0].splits == 19
    ow = {p.overwrite for ps in wr.GROUPS.values() for p in ps}
    assert ow >= {0, 1, 4, 5}
    for ps in wr.GROUPS.values():
        assert {p.bias for p in ps} == {True, False} or len(ps) == 1


@pytest.mark.parametrize('name', list(wr.OPS))
def test_ops_plans(name):
    c = wr.assert_ops(name)
    assert all(i < len(c.probs) and c.probs[i][:3] == c.probs[0][:3] for i in c.shared)
    assert sum(c.fold_launches) == len(c.fold_splits) == sum(not p.in_place for p in c.probs)
    assert list(c.fold_splits) == [p.splits for p in c.probs if not p.in_place]


def test_bad_arguments_are_refused_by_the_host():
    """Every one of these is turned down before any launch, so no device is needed (the pointers are never followed)."""
    import ctypes as C
    t, h = torch.zeros(4096), torch.zeros(4096, dtype=wr.HALF)
    pt, ph = C.c_void_p(t.data_ptr()), C.c_void_p(h.data_ptr())
    ok = [ph, ph, pt, None, pt, 8, 8, 8, 8, 8, None, None, 0]
    for i, v in ((6, 12), (7, 4), (8, 4), (9, 12), (5, 0), (0, None), (4, None), (10, pt)):
        a = list(ok)
        a[i] = v
        assert L().clv_linear_wgrad(*a, None) == -1, f'argument {i} = {v} was accepted'
    assert L().clv_colsum(ph, pt, 8, 12, 16, None) == -1 and L().clv_colsum(ph, pt, 0, 8, 8, None) == -1
    arr = (_lib.ClvWgradEntry * 1)()
    arr[0].M, arr[0].N, arr[0].K = 64, 12, 8
    assert L().clv_linear_wgrad_batch_plan(arr, 1) == -1
    assert L().clv_linear_wgrad_batch_plan(arr, 0) == -1 and L().clv_linear_wgrad_batch_plan(arr, _lib.WGRAD_GROUP_MAX + 1) == -1
    arr[0].N = 8
    assert L().clv_linear_wgrad_batch_plan(arr, 1) == 0
    assert L().clv_linear_wgrad_batch_ss(arr, 1, None, None) == -1             # no operands
    ent = (_lib.ClvFoldEntry * 1)()
    e = ent[0]
    e.partial, e.dw, e.nk, e.e2, e.splits = t.data_ptr(), t.data_ptr(), 8, 16, 0
    assert L().clv_wgrad_fold_batch_ss(ent, 1, None, None) == -1               # no slices
    e.splits, e.nk = 1, 6
    assert L().clv_wgrad_fold_batch_ss(ent, 1, None, None) == -1               # nk not a multiple of 4
    assert L().clv_wgrad_fold_batch_ss(ent, _lib.FOLD_MAX + 1, None, None) == -1


def test_a_retuned_planner_fails_the_claims(monkeypatch):
    """The claims are checked against what the library says, so a planner that says something else must fail them: here the
    library's answers are replaced by those of a retuned one (one slice more)."""
    real = L()

    class Retuned:
        def __getattr__(self, k):
            return getattr(real, k)

        def clv_linear_wgrad_splits(self, M, N, K):
            s = real.clv_linear_wgrad_splits(M, N, K)
            return s + 1 if s > 1 else s

        def clv_linear_wgrad_work_floats(self, M, N, K):
            return self.clv_linear_wgrad_splits(M, N, K) * (N * K + N)

    monkeypatch.setattr(_lib, 'lib', lambda: Retuned())
    with pytest.raises(AssertionError, match='off its path'):
        wr.assert_single('xcd-negative-tail')
    wr.assert_single('inplace-1000')                           # (one slice stays one slice in this retune)
