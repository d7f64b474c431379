"""Retrieval ranks on the device (csrc/retrieval.hip, ops.retrieval_rank, evaluation.recall_on_device) against the
reference's recorded metric values, against exact arithmetic, and against fp64 scores with an a-priori error window.
`-m gpu` only.

The windowed criterion: with device scores within eps of the fp64 scores, the device rank of query i must lie in
[#{j : s_j > s_g + eps}, #{j != g : s_j >= s_g - eps}] (s = row i of the fp64 scores, g its ground truth).  The share
of queries whose window holds more than one value is asserted too (<= 5 %), so wide windows cannot hide a failure."""
import numpy as np
import pytest
import torch

import closed_form as cf
import gutil

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KEYS = ['Recall@1', 'Recall@5', 'Recall@10', 'MR', 'Recall@all']


def _norm64(x):
    x = np.asarray(x, dtype=np.float64)
    n = np.linalg.norm(x, axis=1, keepdims=True)
    n[n == 0] = 1
    return x / n


def _make(Nq, Ng, D, caps, seed):
    """gallery standard normal; query = a * gallery[gt] + noise with a log-uniform in [0.02, 1]: ranks from 0 into the bulk."""
    rng = np.random.default_rng(seed)
    gal = rng.standard_normal((Ng, D)).astype(np.float32)
    if caps > 1:
        assert Nq == Ng * caps
        gt = np.arange(Nq) // caps
    elif Nq == Ng:
        gt = np.arange(Nq)
    else:
        gt = rng.integers(0, Ng, Nq)
    a = np.exp(rng.uniform(np.log(0.02), np.log(1.0), (Nq, 1))).astype(np.float32)
    q = (a * gal[gt] + rng.standard_normal((Nq, D)).astype(np.float32)).astype(np.float32)
    return q, gal, gt.astype(np.int64)


def _check_windowed(q, gal, gt, pass_gt, eps, topk, s64=None):
    from clover_amd import ops
    Nq, Ng = len(q), len(gal)
    if s64 is None:
        s64 = _norm64(q) @ _norm64(gal).T
    gt_dev = torch.from_numpy(gt).to(DEV) if pass_gt else None
    rank, gs, tidx, tsc = ops.retrieval_rank(torch.from_numpy(q).to(DEV), torch.from_numpy(gal).to(DEV), gt=gt_dev,
                                             topk=topk)
    rank, gs = rank.cpu().numpy(), gs.cpu().numpy().astype(np.float64)
    sg = s64[np.arange(Nq), gt]
    lo = (s64 > (sg + eps)[:, None]).sum(1)
    others = np.ones_like(s64, dtype=bool)
    others[np.arange(Nq), gt] = False
    hi = ((s64 >= (sg - eps)[:, None]) & others).sum(1)
    wide = float(np.mean(hi > lo))
    err = np.abs(gs - sg).max()
    print(f'Nq={Nq} Ng={Ng} D={q.shape[1]} eps={eps:.3e} max|gt_score - fp64|={err:.3e} wide windows={100 * wide:.2f}% '
          f'outside={int(((rank < lo) | (rank > hi)).sum())}')
    assert rank.dtype == np.int32 and rank.shape == (Nq,)
    assert err <= eps
    assert np.all((rank >= lo) & (rank <= hi)), np.nonzero((rank < lo) | (rank > hi))[0][:10]
    assert wide <= 0.05, wide
    if topk:
        tidx, tsc = tidx.cpu().numpy(), tsc.cpu().numpy().astype(np.float64)
        assert tidx.shape == tsc.shape == (Nq, topk) and tidx.dtype == np.int32
        k = min(topk, Ng)
        assert np.all(tidx[:, k:] == -1) and np.all(np.isneginf(tsc[:, k:]))              # padding when Ng < K
        assert np.all((tidx[:, :k] >= 0) & (tidx[:, :k] < Ng))
        assert all(len(set(row)) == k for row in tidx[:, :k].tolist())
        picked = np.take_along_axis(s64, tidx[:, :k].astype(np.int64), axis=1)
        assert np.abs(tsc[:, :k] - picked).max() <= eps
        assert np.all(np.diff(tsc[:, :k], axis=1) <= 0)                                   # descending
        # scores within eps of fp64 => the p-th largest device score is within eps of the p-th largest fp64 score
        best = -np.sort(-s64, axis=1)[:, :k]
        assert np.abs(tsc[:, :k] - best).max() <= eps
    return rank


def test_reference_goldens():
    """The five numbers the REAL reference recorded for recall.N{1,7,50,200} (g_finetune.npz; inputs regenerated as
    test_recall_for_video_text_retrieval_goldens does); the zeroed query of N = 7 has all-equal scores: rank 3 by index."""
    from clover_amd import ops
    from clover_amd.evaluation import recall_on_device
    g = gutil.load('g_finetune.npz')
    for N, D in ((1, 8), (7, 16), (50, 32), (200, 64)):
        ve = cf.cf_float(f'recall.N{N}.v', (N, D), 1.0).numpy()
        te = (0.35 * ve + cf.cf_float(f'recall.N{N}.t', (N, D), 1.0).numpy()).astype(np.float32)
        if N == 7:
            te[3] = 0
        m = recall_on_device(torch.from_numpy(ve).to(DEV), torch.from_numpy(te).to(DEV))
        assert list(m) == KEYS
        np.testing.assert_allclose([m[k] for k in KEYS], g[f'recall.N{N}'], rtol=0, atol=1e-9)
        if N == 7:
            rank, gs, _, _ = ops.retrieval_rank(torch.from_numpy(te).to(DEV), torch.from_numpy(ve).to(DEV))
            assert int(rank[3]) == 3 and float(gs[3]) == 0.0


@pytest.fixture(scope='module')
def exact_case():
    """D = 768, Ng = 300: every row has exactly 64 entries of +-1, so its norm is 8, the normalised entries are +-0.125
    and every score is a multiple of 1/64 — exact in fp32 in any summation order.  Rows 17 and 250 copy row 3."""
    rng = np.random.default_rng(20)
    Ng, D = 300, 768
    gal = np.zeros((Ng, D), np.float32)
    for i in range(Ng):
        gal[i, rng.choice(D, 64, replace=False)] = rng.choice([-1.0, 1.0], 64)
    gal[17] = gal[3]
    gal[250] = gal[3]
    extra = np.stack([gal[3], gal[3], gal[17], gal[250], gal[100]])
    q = np.concatenate([gal, extra])
    gt = np.concatenate([np.arange(Ng), [17, 250, 3, 17, 250]]).astype(np.int64)
    s = np.dot(q / np.float32(8), (gal / np.float32(8)).T)
    assert s.dtype == np.float32 and np.array_equal(s * 64, np.round(s * 64))
    order = np.argsort(-s, axis=1, kind='stable')
    return q, gal, gt, s, order


@pytest.mark.parametrize('topk', [1, 10, 16])
def test_exact_arithmetic_bit_for_bit(exact_case, topk):
    from clover_amd import ops
    q, gal, gt, s, order = exact_case
    Nq = len(q)
    rank, gs, tidx, tsc = ops.retrieval_rank(torch.from_numpy(q).to(DEV), torch.from_numpy(gal).to(DEV),
                                             gt=torch.from_numpy(gt).to(DEV), topk=topk)
    want_rank = np.where(order == gt[:, None])[1]
    assert want_rank[3] == 0 and want_rank[17] == 1 and want_rank[250] == 2               # ties on both sides of gt
    assert np.array_equal(rank.cpu().numpy(), want_rank.astype(np.int32))
    assert np.array_equal(gs.cpu().numpy(), s[np.arange(Nq), gt])
    assert np.array_equal(tidx.cpu().numpy(), order[:, :topk].astype(np.int32))
    assert np.array_equal(tsc.cpu().numpy(), np.take_along_axis(s, order[:, :topk], axis=1))
    if topk == 1:                                          # the same ranks without the top-K pass and its LDS detour
        rank0, gs0, none_i, none_s = ops.retrieval_rank(torch.from_numpy(q).to(DEV), torch.from_numpy(gal).to(DEV),
                                                        gt=torch.from_numpy(gt).to(DEV))
        assert none_i is None and none_s is None
        assert torch.equal(rank0, rank) and torch.equal(gs0, gs)


@pytest.mark.parametrize('Nq,Ng,D,caps', [(333, 333, 64, 1), (515, 103, 96, 5), (130, 1030, 36, 1), (1, 1, 4, 1),
                                          (17, 5, 8, 1)])
def test_random_inputs_windowed(Nq, Ng, D, caps):
    """Sizes that are no multiple of the 64 x 64 tile, D no multiple of the 16-deep stage, Nq != Ng with gt, a gallery
    long enough to be split over workgroups, one tile with one element, fewer gallery rows than K.
    eps = 2 (D + 4) 2^-24: the a-priori fp32 bound for a dot product of unit vectors plus the two normalisations."""
    from clover_amd.evaluation import recall_on_device
    q, gal, gt = _make(Nq, Ng, D, caps, seed=Nq * 7 + D)
    eps = 2 * (D + 4) * 2.0 ** -24
    rank = _check_windowed(q, gal, gt, pass_gt=not (Nq == Ng and caps == 1), eps=eps, topk=10)
    if caps > 1:                                           # [N, C, D] captions: gt = i // C inside recall_on_device
        m = recall_on_device(torch.from_numpy(gal).to(DEV), torch.from_numpy(q.reshape(Ng, caps, D)).to(DEV), topk=3)
        assert m['topk'].shape == (Nq, 3)
        assert m['Recall@5'] == float(np.sum(rank < 5)) / Nq * 100 and m['MR'] == np.median(rank) + 1
        assert m['Recall@all'] == m['Recall@1'] + m['Recall@5'] + m['Recall@10'] - m['MR']


@pytest.mark.parametrize('N', [1000, 2049])
def test_real_width_random(N):
    """D = 768, where the a-priori eps would make 21-27 % of the windows wide: eps is measured on the reference
    arithmetic instead, 8 x max|numpy fp32 score - fp64 score| (an MFMA k-chain sums sequentially where numpy sums
    pairwise: a sequential fp32 chain has about 1.5 x numpy's error)."""
    from clover_amd.evaluation import normalize_fn
    q, gal, gt = _make(N, N, 768, 1, seed=N)
    s64 = _norm64(q) @ _norm64(gal).T
    s32 = np.dot(normalize_fn(q), normalize_fn(gal).T)
    assert s32.dtype == np.float32
    eps = 8 * float(np.abs(s32.astype(np.float64) - s64).max())
    _check_windowed(q, gal, gt, pass_gt=False, eps=eps, topk=5, s64=s64)


def test_unsupported_shapes_and_cpu_tensors():
    from clover_amd import _lib, ops
    from clover_amd.ops import _ptr, _stream
    L = _lib.lib()
    q, g = torch.randn(8, 8, device=DEV), torch.randn(8, 8, device=DEV)
    rank = torch.empty(8, device=DEV, dtype=torch.int32)
    gs = torch.empty(8, device=DEV)
    ti, ts = torch.empty(8, 17, device=DEV, dtype=torch.int32), torch.empty(8, 17, device=DEV)
    work = torch.empty(1 << 16, device=DEV, dtype=torch.uint8)
    assert L.clv_retrieval_work_bytes(8, 8, 6, 0) == -2 and L.clv_retrieval_work_bytes(8, 8, 8, 17) == -2
    assert L.clv_retrieval_work_bytes(8, 8, 8, 16) == 2 * 8 * 8 * 4 + 8 * 16 * 8
    assert L.clv_retrieval_rank(_ptr(q), _ptr(g), None, _ptr(rank), _ptr(gs), None, None, _ptr(work), 8, 8, 6, 8, 8, 0,
                                _stream()) == -2                                          # D % 4
    assert L.clv_retrieval_rank(_ptr(q), _ptr(g), None, _ptr(rank), _ptr(gs), _ptr(ti), _ptr(ts), _ptr(work), 8, 8, 8, 8,
                                8, 17, _stream()) == -2                                   # topk > 16
    with pytest.raises(RuntimeError, match='CLV_ERR_UNSUPPORTED'):
        ops.retrieval_rank(q[:, :6].contiguous(), g[:, :6].contiguous())
    with pytest.raises(RuntimeError, match='CLV_ERR_UNSUPPORTED'):
        ops.retrieval_rank(q, g, topk=17)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_rank(q.cpu(), g.cpu())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_rank(q, g, gt=torch.arange(8))
    # a query without ground truth: rank -1, and recall_on_device leaves it out
    gt = torch.tensor([0, 1, -1, 3, 4, 5, 6, 7], device=DEV)
    r, _, _, _ = ops.retrieval_rank(g.clone(), g, gt=gt)
    assert r.tolist() == [0, 0, -1, 0, 0, 0, 0, 0]
    # a row stride larger than D (a column slice of a wider tensor) is read in place
    wide = torch.randn(8, 24, device=DEV)
    r2, s2, _, _ = ops.retrieval_rank(wide[:, :8], g)
    r3, s3, _, _ = ops.retrieval_rank(wide[:, :8].contiguous(), g)
    assert torch.equal(r2, r3) and torch.equal(s2, s3)
