"""Dual-softmax re-scoring on the device (clv_retrieval_col_stats, clv_retrieval_rank_prior; ops.retrieval_rank(...,
dual_softmax=T); the DSL_* keys of the evaluation module) against exact arithmetic, and against fp64 with the a-priori
bounds of tests/RETRIEVAL_DSL_ERROR_BUDGET.md (tests/retrieval_dsl_ref.py).  `-m gpu` only.

The windowed criterion is that of tests/test_retrieval_gpu.py with a bound per element: with every device s' within e_ij
of the fp64 s', the device rank of query i lies in [#{j : certainly above gt}, #{j != g : possibly above or tied}].  The
share of windows that hold more than one value is capped (tests/test_retrieval_dsl_cpu.py asserts the cap, and that numpy
in fp32 meets the same windows)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import retrieval_dsl_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ['Recall@1', 'Recall@5', 'Recall@10', 'MR', 'Recall@all']
DSL = ['DSL_' + k for k in PLAIN]


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared reference arrays are read-only


@pytest.fixture(scope='module')
def exact_case():
    """The construction of test_retrieval_gpu.exact_case (64 entries of +-1 per row of D = 768: norm 8, every score a
    multiple of 1/64) with Nq = 512 = 2^9 queries: the 300 gallery rows, the five extra queries around the duplicated rows
    3 = 17 = 250 (ties on both sides of gt), and 207 more copies.  With T = 0 the prior is exactly 1 / 512."""
    from clover_amd import ops
    rng = np.random.default_rng(20)
    Ng, D = 300, 768
    gal = np.zeros((Ng, D), np.float32)
    for i in range(Ng):
        gal[i, rng.choice(D, 64, replace=False)] = rng.choice([-1.0, 1.0], 64)
    gal[17] = gal[3]
    gal[250] = gal[3]
    more = rng.integers(0, Ng, 207)
    q = np.concatenate([gal, np.stack([gal[3], gal[3], gal[17], gal[250], gal[100]]), gal[more]])
    gt = np.concatenate([np.arange(Ng), [17, 250, 3, 17, 250], rng.integers(0, Ng, 207)]).astype(np.int64)
    assert len(q) == 512
    qd, gd, gtd = _dev(q), _dev(gal), _dev(gt)
    plain = {k: ops.retrieval_rank(qd, gd, gt=gtd, topk=k) for k in (0, 1, 10, 16)}
    return qd, gd, gtd, plain


def test_exact_column_statistics(exact_case):
    from clover_amd import ops
    qd, gd, _, _ = exact_case
    cmax, csum = ops.retrieval_col_stats(qd, gd, 0.0)
    assert cmax.shape == csum.shape == (300,) and cmax.dtype == csum.dtype == torch.float32
    assert bool((cmax == 0).all()) and bool((csum == 512).all())


@pytest.mark.parametrize('topk', [0, 1, 10, 16])
def test_exact_arithmetic_bit_for_bit(exact_case, topk):
    """T = 0: s' = s / 512 exactly, so the order is the plain one and every output equals clv_retrieval_rank's, the scores
    after an exact scaling."""
    from clover_amd import ops
    qd, gd, gtd, plain = exact_case
    rank0, gs0, tidx0, tsc0 = plain[topk]
    rank, gs, tidx, tsc = ops.retrieval_rank(qd, gd, gt=gtd, topk=topk, dual_softmax=0.0)
    assert rank0[3] == 0 and rank0[17] == 1 and rank0[250] == 2                          # ties on both sides of gt
    assert rank.dtype == torch.int32 and torch.equal(rank, rank0)
    assert torch.equal(gs * 512, gs0)
    if topk:
        assert torch.equal(tidx, tidx0) and torch.equal(tsc * 512, tsc0)
    else:
        assert tidx is None and tsc is None


STAT_SIZES = [(1, 1, 4),            # one tile with one element
              (65, 65, 36),         # one tile plus one row; D no multiple of the 16-deep stage; 65 queries: the smallest
                                    # number that is split over workgroups (two chunks of one 64-query tile)
              (64, 65, 36),         # ... and one fewer: a single chunk
              (130, 1030, 96),      # gallery split over 17 workgroups
              (2049, 70, 64)]       # 33 query chunks: the prior spans all queries


@pytest.mark.parametrize('T', R.TEMPERATURES)
@pytest.mark.parametrize('Nq,Ng,D', STAT_SIZES)
def test_column_statistics_against_fp64(Nq, Ng, D, T):
    from clover_amd import ops
    q, gal, gt = R.make(Nq, Ng, D, 1, seed=Nq * 7 + D)
    q = q.copy()
    if Nq > 1:
        q[Nq // 2] = 0                                      # an all-zero query: s = 0, it adds exp(0 - m_j) to every l_j
    s64, m64, l64, p64, sp64 = R.ref64(q, gal, T)
    qd, gd = _dev(q), _dev(gal)
    cmax, csum = ops.retrieval_col_stats(qd, gd, T)
    again = ops.retrieval_col_stats(qd, gd, T)
    assert torch.equal(cmax, again[0]) and torch.equal(csum, again[1])                   # one fixed order of the merge
    m, l = cmax.cpu().numpy().astype(np.float64), csum.cpu().numpy().astype(np.float64)
    es = R.eps_s(D)
    em, el = np.abs(m - m64).max(), (np.abs(l - l64) / l64).max()
    print(f'Nq={Nq} Ng={Ng} D={D} T={T:g} max|m - m64|={em:.3e} (bound {T * es:.3e}, ratio {em / (T * es):.3f}) '
          f'max rel l={el:.3e} (bound {R.eps_l(Nq, es, T):.3e}, ratio {el / R.eps_l(Nq, es, T):.3f})')
    assert m.shape == l.shape == (Ng,)
    assert em <= T * es
    assert el <= R.eps_l(Nq, es, T)
    assert np.all(l >= 1)
    if Nq > 1:
        zero = Nq // 2
        g0 = int(gt[zero])
        _, gs, _, _ = ops.retrieval_rank(qd, gd, gt=_dev(gt), dual_softmax=T)
        assert float(gs[zero]) == 0.0                                                    # its own s' is 0
        # ... and l_j counts it: without that row the sum is smaller by exp(-m_j)
        without = l64[g0] - np.exp(-m64[g0])
        assert abs(l[g0] - l64[g0]) < abs(l[g0] - without) or np.exp(-m64[g0]) < R.eps_l(Nq, es, T) * l64[g0]


@pytest.mark.parametrize('T', R.TEMPERATURES)
@pytest.mark.parametrize('case', R.WINDOW_CASES + [R.WIDE_CASE], ids=lambda c: 'x'.join(map(str, c[:3])))
def test_ranks_windowed(case, T):
    from clover_amd import ops
    Nq, Ng, D, caps, topk, _ = case
    c = R.window_case(case, T)
    gt, sp64, e = c['gt'], c['sp64'], c['e']
    gt_dev = _dev(gt) if not (Nq == Ng and caps == 1) else None
    rank, gs, tidx, tsc = ops.retrieval_rank(_dev(c['q']), _dev(c['gal']), gt=gt_dev, topk=topk, dual_softmax=T)
    rank, gs = rank.cpu().numpy(), gs.cpu().numpy().astype(np.float64)
    rows = np.arange(Nq)
    err = np.abs(gs - sp64[rows, gt])
    outside = (rank < c['lo']) | (rank > c['hi'])
    print(f'Nq={Nq} Ng={Ng} D={D} T={T:g} eps_s={c["eps_s"]:.3e} eps_r={R.eps_r(Nq, c["eps_s"], T):.3e} '
          f'max |gt_score - fp64| / e={float((err / e[rows, gt]).max()):.3f} wide windows={100 * c["wide"]:.2f}% '
          f'outside={int(outside.sum())}')
    assert rank.dtype == np.int32 and rank.shape == (Nq,)
    assert np.all(err <= e[rows, gt])
    assert not outside.any(), np.nonzero(outside)[0][:10]
    assert c['wide'] <= R.WIDE_CAP, c['wide']
    # top-K: the re-scored order
    tidx, tsc = tidx.cpu().numpy(), tsc.cpu().numpy().astype(np.float64)
    assert tidx.shape == tsc.shape == (Nq, topk) and tidx.dtype == np.int32
    k = min(topk, Ng)
    assert np.all(tidx[:, k:] == -1) and np.all(np.isneginf(tsc[:, k:]))                  # padding when Ng < K
    assert np.all((tidx[:, :k] >= 0) & (tidx[:, :k] < Ng))
    assert all(len(set(row)) == k for row in tidx[:, :k].tolist())
    picked = tidx[:, :k].astype(np.int64)
    assert np.all(np.abs(tsc[:, :k] - np.take_along_axis(sp64, picked, axis=1)) <= np.take_along_axis(e, picked, axis=1))
    assert np.all(np.diff(tsc[:, :k], axis=1) <= 0)                                       # descending
    # every device value within e of fp64 => the p-th largest device value lies between the p-th largest of s'64 - e and
    # the p-th largest of s'64 + e
    top_up, top_dn = -np.sort(-(sp64 + e), axis=1)[:, :k], -np.sort(-(sp64 - e), axis=1)[:, :k]
    assert np.all(tsc[:, :k] <= top_up) and np.all(tsc[:, :k] >= top_dn)
    ratio = np.maximum(tsc[:, :k] - top_up, top_dn - tsc[:, :k]).max()
    print(f'  top-{k}: worst distance past the bound of the k best fp64 values {ratio:.3e} (<= 0 passes)')


def _tight_case():
    """24 videos, 48 captions in counts of 1, 3, 2: well separated, so every rank window holds one value."""
    rng = np.random.default_rng(11)
    counts = np.array([1, 3, 2] * 8)
    v = rng.standard_normal((24, 16)).astype(np.float32)
    gt = np.repeat(np.arange(24), counts)
    t = (v[gt] + 1.5 * rng.standard_normal((48, 16))).astype(np.float32)
    return v, t, counts, gt


def _numpy_dsl_ranks(q, gal, gt, T):
    """The numpy restatement's ranks, after checking that the fp64 windows leave no choice."""
    s64, _, _, p64, sp64 = R.ref64(q, gal, T)
    lo, hi = R.windows(sp64, R.bound(s64, p64, len(q), R.eps_s(q.shape[1]), T), gt)
    assert np.array_equal(lo, hi)                                                         # all tight
    ind = R.stable_ranks(R.restate32(q, gal, T)[1], gt)
    assert np.array_equal(ind, lo)
    return ind


def test_recall_on_device_adds_dsl_keys():
    from clover_amd.evaluation import recall_on_device
    from clover_amd.evaluation.retrieval import _recall_keys
    T = 20.0
    v, t, _, _ = _tight_case()
    t2 = t.reshape(24, 2, 16)                              # [N, C, D]: two captions per video, gt = i // 2
    for text, q, gt in ((t[:24], t[:24], np.arange(24)), (t2, t, np.arange(48) // 2)):
        plain = recall_on_device(_dev(v), _dev(text), topk=3)
        both = recall_on_device(_dev(v), _dev(text), topk=3, dual_softmax=T)
        assert list(both) == PLAIN + ['topk'] + DSL + ['dsl_topk']
        assert all(both[k] == plain[k] for k in PLAIN) and np.array_equal(both['topk'], plain['topk'])
        ind = _numpy_dsl_ranks(q, v, gt, T)
        want = _recall_keys(ind, 'DSL_')
        assert all(both[k] == want[k] for k in want)
        assert both['DSL_Recall@all'] == want['DSL_Recall@1'] + want['DSL_Recall@5'] + want['DSL_Recall@10'] - want['DSL_MR']
        sp32 = R.restate32(q, v, T)[1]
        assert both['dsl_topk'].shape == (len(q), 3)
        assert np.array_equal(both['dsl_topk'], np.argsort(-sp32, axis=1, kind='stable')[:, :3])
        assert 'dsl_topk' not in recall_on_device(_dev(v), _dev(text), dual_softmax=T)


def test_recall_varied_on_device_adds_dsl_keys():
    from clover_amd.evaluation import evaluate_retrieval, recall_varied_on_device
    from clover_amd.evaluation.retrieval import _recall_keys
    T = 20.0
    v, t, counts, gt = _tight_case()
    plain = recall_varied_on_device(_dev(v), _dev(t), _dev(counts), v2t=True)
    both = recall_varied_on_device(_dev(v), _dev(t), _dev(counts), dual_softmax=T)
    assert list(both) == PLAIN[:4] + DSL[:4]
    assert all(both[k] == plain[k] for k in PLAIN[:4])
    want = _recall_keys(_numpy_dsl_ranks(t, v, gt, T), 'DSL_')
    assert {k: both[k] for k in DSL[:4]} == want
    res = dict(video_embd=_dev(v), text_embd=_dev(t), counts=_dev(counts))
    assert evaluate_retrieval(res, ['recall_for_video_text_retrieval_varied'], dual_softmax=T) == both
    with pytest.raises(ValueError, match='V2T_'):
        recall_varied_on_device(_dev(v), _dev(t), _dev(counts), v2t=True, dual_softmax=T)
    with pytest.raises(ValueError, match='multiple choice'):
        evaluate_retrieval(dict(res, label=_dev(np.zeros(24, np.int64))), ['video_qa_mc'], dual_softmax=T)


def test_eval_hook_records_dsl_keys(tmp_path):
    """One evaluation of the tiny retrieval model through the hook: both key families, the plain one unchanged."""
    from clover_amd.runner import CloverRunner, EvalHook
    from test_engine_gpu import make_finetune_model
    from test_eval_hook_gpu import val_loader
    m = make_finetune_model()
    loader = val_loader()
    runner = CloverRunner(m, work_dir=str(tmp_path), max_epochs=1)
    plain, hook = EvalHook(loader, save_best=None), EvalHook(loader, dual_softmax=20.0, save_best=None)
    plain.after_train_epoch(runner)
    hook.after_train_epoch(runner)
    rec = hook.records[-1]
    assert rec['epoch'] == 1 and 'DSL_Recall@1' in rec and set(DSL) <= set(rec)
    assert all(np.isfinite(rec[k]) for k in DSL) and 0 <= rec['DSL_Recall@1'] <= 100
    assert {k: rec[k] for k in PLAIN} == {k: plain.records[-1][k] for k in PLAIN}


@pytest.mark.skipif(os.environ.get('CLOVER_HALF', 'f16').lower() == 'bf16', reason='this process already runs the bf16 build')
def test_ranks_in_the_bf16_build():
    """libclover_hip.so (CLOVER_HALF=bf16) exports and runs the same entries: one windowed case in a child process."""
    env = dict(os.environ, CLOVER_HALF='bf16')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu', 'tests/test_retrieval_dsl_gpu.py', '-k',
                        'test_ranks_windowed and 515x103x96 and 20.0'], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert '1 passed' in r.stdout


def test_unsupported_shapes_bad_temperatures_and_cpu_tensors():
    from clover_amd import _lib, ops
    from clover_amd.ops import _ptr, _stream
    L = _lib.lib()
    q, g = torch.randn(8, 8, device=DEV), torch.randn(8, 8, device=DEV)
    rank = torch.empty(8, device=DEV, dtype=torch.int32)
    gs, cm, cl = torch.empty(8, device=DEV), torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    ti, ts = torch.empty(8, 17, device=DEV, dtype=torch.int32), torch.empty(8, 17, device=DEV)
    work = torch.empty(1 << 16, device=DEV, dtype=torch.uint8)
    assert L.clv_retrieval_col_stats_work_bytes(8, 8, 6) == -2 and L.clv_retrieval_rank_prior_work_bytes(8, 8, 8, 17) == -2
    assert L.clv_retrieval_rank_prior_work_bytes(8, 8, 8, 16) == L.clv_retrieval_work_bytes(8, 8, 8, 16)

    def stats(D=8, T=1.0, cmax=cm):
        return L.clv_retrieval_col_stats(_ptr(q), _ptr(g), 8, 8, D, 8, 8, T, _ptr(cmax), _ptr(cl), _ptr(work), _stream())

    def prior(D=8, topk=0, T=1.0, cmax=cm):
        return L.clv_retrieval_rank_prior(_ptr(q), _ptr(g), None, _ptr(rank), _ptr(gs), _ptr(ti), _ptr(ts), _ptr(work), 8, 8,
                                          D, 8, 8, topk, _ptr(cmax), _ptr(cl), T, _stream())
    assert stats(D=6) == -2 and prior(D=6) == -2                                          # D % 4
    assert prior(topk=17) == -2                                                           # topk > 16
    for bad in (-1.0, float('nan'), float('inf')):
        assert stats(T=bad) == -1 and prior(T=bad) == -1                                  # T finite and >= 0
    assert stats(cmax=None) == -1 and prior(cmax=None) == -1
    assert stats() == 0 and prior() == 0 and prior(topk=16) == 0
    with pytest.raises(RuntimeError, match='CLV_ERR_UNSUPPORTED'):
        ops.retrieval_rank(q[:, :6].contiguous(), g[:, :6].contiguous(), dual_softmax=20.0)
    with pytest.raises(RuntimeError, match='CLV_ERR_UNSUPPORTED'):
        ops.retrieval_rank(q, g, topk=17, dual_softmax=20.0)
    with pytest.raises(RuntimeError, match='CLV_ERR_ARG'):
        ops.retrieval_rank(q, g, dual_softmax=-1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_rank(q.cpu(), g.cpu(), dual_softmax=20.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_rank(q, g, gt=torch.arange(8), dual_softmax=20.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_col_stats(q.cpu(), g, 20.0)
    # a query without ground truth: rank -1, NaN score, and it still takes part in the prior of the others
    gt = torch.tensor([0, 1, -1, 3, 4, 5, 6, 7], device=DEV)
    r, s, _, _ = ops.retrieval_rank(g.clone(), g, gt=gt, dual_softmax=20.0)
    assert r.tolist() == [0, 0, -1, 0, 0, 0, 0, 0] and bool(torch.isnan(s[2])) and bool(torch.isfinite(s[[0, 1, 3]]).all())
    # a row stride larger than D is read in place
    wide = torch.randn(8, 24, device=DEV)
    r2, s2, _, _ = ops.retrieval_rank(wide[:, :8], g, dual_softmax=20.0)
    r3, s3, _, _ = ops.retrieval_rank(wide[:, :8].contiguous(), g, dual_softmax=20.0)
    assert torch.equal(r2, r3) and torch.equal(s2, s3)
