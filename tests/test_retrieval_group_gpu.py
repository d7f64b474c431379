"""The best gallery row inside a per-query range and its rank on the device (csrc/retrieval.hip RT_BEST,
ops.retrieval_group_best, evaluation.mc_acc_on_device / recall_varied_on_device) against exact arithmetic, against
ops.retrieval_rank, and against fp64 scores with an a-priori error window.  `-m gpu` only.

The windowed criterion: with device scores within eps of the fp64 scores, the device's best row of query i must lie in
{j in range : s_j >= max - 2 eps} (s = row i of the fp64 scores) and its score within eps of the fp64 maximum.  The
share of queries for which that set holds more than one row is asserted too (<= 5 %), so wide sets cannot hide a
failure."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _norm64(x, eps=0.0):
    x = np.asarray(x, dtype=np.float64)
    n = np.maximum(np.linalg.norm(x, axis=1, keepdims=True), eps)
    n[n == 0] = 1
    return x / n


def _best_in_range(s, lo, hi):
    """numpy's answer on a score matrix: (first argmax inside [lo, hi), the maximum); -1 / NaN for a range that is
    empty or leaves the gallery."""
    Nq, Ng = s.shape
    idx, val = np.full(Nq, -1, np.int32), np.full(Nq, np.nan, s.dtype)
    for i in range(Nq):
        if 0 <= lo[i] < hi[i] <= Ng:
            idx[i] = lo[i] + int(np.argmax(s[i, lo[i]:hi[i]]))
            val[i] = s[i, idx[i]]
    return idx, val


def _dev(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in xs]


@pytest.fixture(scope='module')
def exact_case():
    """test_retrieval_gpu.py's construction: D = 768, every row has exactly 64 entries of +-1, so its norm is 8, the
    normalised entries are +-0.125 and every score is a multiple of 1/64 — exact in fp32 in any summation order (and the
    eps = 1e-8 of sim_matrix changes nothing).  70 videos (more than one 64-query block), 350 texts = 5 candidates each;
    a handful of scores per row coincide by chance, and candidates are duplicated on purpose: texts 16 and 18 copy video 3
    (a tie at the maximum 1 inside video 3's range), texts 62 and 64 are equal (a tie across the 64-column tile
    boundary inside video 12's range [60, 65))."""
    rng = np.random.default_rng(21)
    Nq, Ng, D = 70, 350, 768

    def rows(n):
        x = np.zeros((n, D), np.float32)
        for i in range(n):
            x[i, rng.choice(D, 64, replace=False)] = rng.choice([-1.0, 1.0], 64)
        return x
    q, gal = rows(Nq), rows(Ng)
    gal[16] = q[3]
    gal[18] = q[3]
    gal[62] = q[12]
    gal[64] = q[12]
    s = np.dot(q / np.float32(8), (gal / np.float32(8)).T)
    assert s.dtype == np.float32 and np.array_equal(s * 64, np.round(s * 64))
    return q, gal, s


def _exact_ranges(kind, Nq, Ng):
    if kind == 'candidates':                                       # multiple choice: [5 i, 5 i + 5)
        lo = np.arange(Nq) * 5
        return lo, lo + 5
    if kind == 'unequal':                                          # lengths 1..7 back to back, then the special cases
        ln = np.arange(Nq) % 7 + 1
        hi = np.cumsum(ln)
        lo = hi - ln
        assert hi[-1] <= Ng and any(l // 64 != (h - 1) // 64 for l, h in zip(lo, hi))       # some straddle a tile boundary
        lo[5], hi[5] = 40, 40                                      # empty
        lo[6], hi[6] = 50, 45                                      # empty (hi < lo)
        lo[7], hi[7] = 346, 351                                    # leaves the gallery
        lo[8], hi[8] = -1, 3
        lo[9], hi[9] = 0, Ng                                       # everything
        lo[69], hi[69] = 349, 350                                  # the last column alone
        return lo, hi
    return None, None


@pytest.mark.parametrize('kind', ['candidates', 'unequal', 'whole'])
def test_exact_arithmetic_bit_for_bit(exact_case, kind):
    from clover_amd import ops
    q, gal, s = exact_case
    Nq, Ng = s.shape
    lo, hi = _exact_ranges(kind, Nq, Ng)
    want_idx, want_val = _best_in_range(s, *((lo, hi) if lo is not None else (np.zeros(Nq, int), np.full(Nq, Ng))))
    qd, gd = _dev(q, gal)
    lod, hid = _dev(lo, hi) if lo is not None else (None, None)
    for eps in (0.0, 1e-8):
        idx, val, rank = ops.retrieval_group_best(qd, gd, lod, hid, want_rank=True, eps=eps)
        assert idx.dtype == torch.int32 and val.dtype == torch.float32 and rank.dtype == torch.int32
        assert np.array_equal(idx.cpu().numpy(), want_idx)
        assert np.array_equal(val.cpu().numpy(), want_val, equal_nan=True)
        order = np.argsort(-s, axis=1, kind='stable')
        want_rank = np.where(want_idx >= 0, np.argmax(order == want_idx[:, None], axis=1), -1)
        assert np.array_equal(rank.cpu().numpy(), want_rank.astype(np.int32))
        idx2, val2, none = ops.retrieval_group_best(qd, gd, lod, hid, eps=eps)              # without the rank launches
        assert none is None and torch.equal(idx2, idx) and np.array_equal(val2.cpu().numpy(), want_val, equal_nan=True)
    if kind == 'candidates':
        assert want_idx[3] == 16 and want_val[3] == 1.0 and want_idx[12] == 62              # the first of the tied rows
    if kind == 'unequal':
        assert list(want_idx[5:9]) == [-1] * 4 and want_idx[69] == 349


@pytest.mark.parametrize('Nq,Ng,D', [(130, 1030, 36), (17, 5, 8)])
def test_rank_is_retrieval_rank_of_best(Nq, Ng, D):
    """The rank output is clv_retrieval_rank's with gt = best_idx (a gallery split over chunks; one tile of 5 columns)."""
    from clover_amd import ops
    g = torch.Generator().manual_seed(Nq + D)
    q, gal = torch.randn(Nq, D, generator=g).to(DEV), torch.randn(Ng, D, generator=g).to(DEV)
    ln = torch.randint(1, min(6, Ng) + 1, (Nq,), generator=g)
    lo = (torch.rand(Nq, generator=g) * (Ng - ln + 1)).long().clamp(0, Ng - 1)
    hi = torch.minimum(lo + ln, torch.tensor(Ng))
    for rng in ((lo.to(DEV), hi.to(DEV)), (None, None)):
        idx, val, rank = ops.retrieval_group_best(q, gal, *rng, want_rank=True)
        assert int(idx.min()) >= 0
        if rng[0] is not None:
            assert bool(((idx >= rng[0]) & (idx < rng[1])).all())
        ref_rank, ref_score, _, _ = ops.retrieval_rank(q, gal, gt=idx)
        assert torch.equal(rank, ref_rank) and torch.equal(val, ref_score)
        if rng[0] is None:
            assert int(rank.max()) == 0                           # the best row of the whole gallery is first


def _make_groups(Nq, Ng, D, lengths, seed):
    """videos standard normal; the ranges have the given lengths in turn, back to back when they fill the gallery and at
    random places otherwise; the gallery is noise except one row per range = a * video + noise with a log-uniform in
    [0.02, 1] (test_retrieval_gpu._make): the right candidate wins clearly, narrowly or not at all."""
    rng = np.random.default_rng(seed)
    ln = np.resize(np.asarray(lengths), Nq)
    lo = np.cumsum(ln) - ln if ln.sum() == Ng else rng.integers(0, Ng - ln + 1)
    hi = lo + ln
    q = rng.standard_normal((Nq, D)).astype(np.float32)
    gal = rng.standard_normal((Ng, D)).astype(np.float32)
    a = np.exp(rng.uniform(np.log(0.02), np.log(1.0), Nq)).astype(np.float32)
    pos = lo + rng.integers(0, ln)
    gal[pos] += a[:, None] * q
    return q, gal, lo, hi


def _window_sets(s64, lo, hi, eps):
    """-> (per query: the rows of its range within 2 eps of the range's fp64 maximum, the maxima)."""
    sets, mx = [], np.empty(len(s64))
    for i in range(len(s64)):
        seg = s64[i, lo[i]:hi[i]]
        mx[i] = seg.max()
        sets.append(lo[i] + np.nonzero(seg >= mx[i] - 2 * eps)[0])
    return sets, mx


def _check_windowed(q, gal, lo, hi, eps, s64, norm_eps=0.0):
    from clover_amd import ops
    sets, mx = _window_sets(s64, lo, hi, eps)
    wide = float(np.mean([len(x) > 1 for x in sets]))
    idx, val, _ = ops.retrieval_group_best(*_dev(q, gal, lo, hi), eps=norm_eps)
    idx, val = idx.cpu().numpy(), val.cpu().numpy().astype(np.float64)
    err = np.abs(val - mx).max()
    outside = [i for i in range(len(sets)) if idx[i] not in sets[i]]
    print(f'Nq={len(q)} Ng={len(gal)} D={q.shape[1]} eps={eps:.3e} max|best_score - fp64 max|={err:.3e} '
          f'wide sets={100 * wide:.2f}% outside={len(outside)}')
    assert err <= eps
    assert not outside, outside[:10]
    assert wide <= 0.05, wide


@pytest.mark.parametrize('Nq,Ng,D,lengths', [(70, 350, 64, [5]), (333, 1000, 96, [1, 2, 3, 4, 5, 6])])
def test_random_inputs_windowed(Nq, Ng, D, lengths):
    """Ranges of 5 back to back (multiple choice) and ranges of 1-6 anywhere in a gallery of 16 tiles; eps = 2 (D + 4) 2^-24: the a-priori fp32
    bound for a dot product of unit vectors plus the two normalisations (test_retrieval_gpu.py)."""
    q, gal, lo, hi = _make_groups(Nq, Ng, D, lengths, seed=Nq * 7 + D)
    eps = 2 * (D + 4) * 2.0 ** -24
    _check_windowed(q, gal, lo, hi, eps, _norm64(q) @ _norm64(gal).T)
    _check_windowed(q, gal, lo, hi, eps, _norm64(q) @ _norm64(gal).T, norm_eps=1e-8)        # no norm is near 1e-8


def test_real_width_random():
    """D = 768, where the a-priori eps is too loose to separate candidates: eps is measured on the reference arithmetic
    instead, 8 x max|numpy fp32 score - fp64 score| (test_retrieval_gpu.test_real_width_random: an MFMA k-chain sums
    sequentially where numpy sums pairwise)."""
    from clover_amd.evaluation import normalize_fn
    q, gal, lo, hi = _make_groups(130, 650, 768, [5], seed=768)
    s64 = _norm64(q) @ _norm64(gal).T
    s32 = np.dot(normalize_fn(q), normalize_fn(gal).T)
    assert s32.dtype == np.float32
    eps = 8 * float(np.abs(s32.astype(np.float64) - s64).max())
    _check_windowed(q, gal, lo, hi, eps, s64)


def test_normalisation_eps():
    """sim_matrix's 1 / max(norm, eps) (accuracy.py:385-394) against fp64: a query of norm ~1e-9 keeps a tenth of its
    cosine at eps = 1e-8 and all of it at eps = 0; an all-zero query scores 0 everywhere: the first row of its range."""
    from clover_amd import ops
    rng = np.random.default_rng(8)
    D = 8
    gal = rng.uniform(0.5, 1.5, (12, D)).astype(np.float32)                   # positive entries: no cancellation
    q = rng.uniform(0.5, 1.5, (3, D)).astype(np.float32)
    q[1] *= np.float32(1e-9 / np.linalg.norm(q[1]))
    q[2] = 0
    assert 0.5e-9 < np.linalg.norm(q[1].astype(np.float64)) < 2e-9
    lo, hi = np.array([2, 4, 7]), np.array([9, 11, 10])
    for eps in (1e-8, 0.0):
        s64 = _norm64(q, eps) @ _norm64(gal, eps).T
        want_idx, want_val = _best_in_range(s64, lo, hi)
        idx, val, _ = ops.retrieval_group_best(*_dev(q, gal, lo, hi), eps=eps)
        idx, val = idx.cpu().numpy(), val.cpu().numpy().astype(np.float64)
        print(f'eps={eps}: device {val}, fp64 {want_val}')
        assert np.all(np.abs(val[:2] - want_val[:2]) <= 1e-6 * np.abs(want_val[:2]))
        assert (want_val[1] < 0.11) == (eps > 0)                  # scaled by norm / eps ~ 0.1, or to unit norm
        # the two real queries pick fp64's row unless fp64's runner-up is within the same 1e-6
        for i in range(2):
            assert s64[i, idx[i]] >= want_val[i] * (1 - 2e-6)
        assert idx[2] == lo[2] and val[2] == 0.0


def test_metrics_on_the_exact_case(exact_case):
    from clover_amd.evaluation import (acc_for_msrvtt_mc, mc_acc_on_device, recall_for_video_text_retrieval_varied,
                                       recall_varied_on_device)
    q, gal, s = exact_case
    Nq = len(q)
    rng = np.random.default_rng(4)
    want_pred = _best_in_range(s, np.arange(Nq) * 5, np.arange(Nq) * 5 + 5)[0] - np.arange(Nq) * 5
    label = np.where(rng.random(Nq) < 0.5, want_pred, rng.integers(0, 5, Nq))
    host = acc_for_msrvtt_mc(q, gal, label)
    qd, gd = _dev(q, gal)
    assert 0.4 < host['acc'] < 1.0
    assert mc_acc_on_device(qd, gd, label) == host                                          # [N*C, D]
    got = mc_acc_on_device(qd, gd.reshape(Nq, 5, -1), torch.from_numpy(label).to(DEV), return_pred=True)    # [N, C, D]
    assert got['acc'] == host['acc'] and np.array_equal(got['pred'], want_pred)

    counts = np.arange(Nq) % 4 + 1                                                          # 1 2 3 4 1 2 ...
    texts = gal[:counts.sum()]
    host = recall_for_video_text_retrieval_varied(q, texts, counts)
    td = gd[:len(texts)]
    assert recall_varied_on_device(qd, td, counts) == host
    both = recall_varied_on_device(qd, td, torch.from_numpy(counts).to(DEV), v2t=True)
    assert {k: both[k] for k in host} == host
    # video -> text by numpy: the position of the video's best caption in the stable descending order of its row
    sv = s[:, :len(texts)]
    hi = np.cumsum(counts)
    best = _best_in_range(sv, hi - counts, hi)[0]
    ind = np.argmax(np.argsort(-sv, axis=1, kind='stable') == best[:, None], axis=1)
    want = {'V2T_Recall@1': float(np.sum(ind == 0)) / Nq * 100, 'V2T_Recall@5': float(np.sum(ind < 5)) / Nq * 100,
            'V2T_Recall@10': float(np.sum(ind < 10)) / Nq * 100, 'V2T_MR': np.median(ind) + 1}
    assert {k: both[k] for k in want} == want and len(both) == 8


def test_unsupported_shapes_and_strides():
    from clover_amd import _lib, ops
    from clover_amd.ops import _ptr, _stream
    L = _lib.lib()
    q, g = torch.randn(8, 8, device=DEV), torch.randn(8, 8, device=DEV)
    bi, bs = torch.empty(8, device=DEV, dtype=torch.int32), torch.empty(8, device=DEV)
    work = torch.empty(1 << 16, device=DEV, dtype=torch.uint8)
    assert L.clv_retrieval_group_work_bytes(8, 8, 6) == -2 and L.clv_retrieval_group_work_bytes(8, 8, 4100) == -2
    assert L.clv_retrieval_group_work_bytes(8, 8, 8) == 2 * 8 * 8 * 4 + 8 * 8
    for D in (6, 4100):                                                    # D % 4, D > 4096: refused before any launch
        assert L.clv_retrieval_group_best(_ptr(q), _ptr(g), None, None, _ptr(bi), _ptr(bs), None, _ptr(work), 8, 8, D, D,
                                          D, 0.0, _stream()) == -2
    with pytest.raises(RuntimeError, match='CLV_ERR_UNSUPPORTED'):
        ops.retrieval_group_best(q[:, :6].contiguous(), g[:, :6].contiguous())
    with pytest.raises(RuntimeError, match='CLV_ERR_UNSUPPORTED'):
        ops.retrieval_group_best(torch.zeros(2, 4100, device=DEV), torch.zeros(2, 4100, device=DEV))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_group_best(q, g, lo=torch.zeros(8, dtype=torch.int64), hi=torch.ones(8, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.retrieval_group_best(q, g, lo=torch.zeros(8, device=DEV, dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.retrieval_group_best(q.half(), g.half())
    # a row stride larger than D (a column slice of a wider tensor) is read in place; int64 ranges are converted
    wide = torch.randn(8, 24, device=DEV)
    lo, hi = torch.tensor([0, 1, 2, 3, 0, 0, 6, 7], device=DEV), torch.tensor([3, 4, 8, 4, 8, 1, 8, 8], device=DEV)
    a = ops.retrieval_group_best(wide[:, :8], g, lo, hi, want_rank=True)
    b = ops.retrieval_group_best(wide[:, :8].contiguous(), g, lo.int(), hi.int(), want_rank=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a[0].tolist()[3] == 3 and a[0].tolist()[5] == 0 and a[0].tolist()[7] == 7       # ranges of one row
