"""Host side of the dual-softmax (DSL) re-scoring of retrieval: the numpy restatement on cases worked out by hand, the
``DSL_*`` keys of evaluate_retrieval / EvalHook on host results, the two refusals, the config and the CLI flag, the new
library entry points as far as they go without a device, and the condition the GPU tests rest on: the numpy fp32
restatement alone stays inside the rank windows of tests/retrieval_dsl_ref.py, whose wide share stays under the cap."""
import ctypes
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

import retrieval_dsl_ref as R
from clover_amd.evaluation import (dual_softmax_scores, evaluate_retrieval, mc_acc_on_device,
                                   recall_for_video_text_retrieval, recall_for_video_text_retrieval_varied,
                                   recall_varied_on_device)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ['Recall@1', 'Recall@5', 'Recall@10', 'MR', 'Recall@all']
DSL = ['DSL_Recall@1', 'DSL_Recall@5', 'DSL_Recall@10', 'DSL_MR', 'DSL_Recall@all']


def test_dual_softmax_scores_against_loops():
    s = np.array([[0.9, -0.2, 0.3, 0.0],
                  [0.1, 0.8, -0.5, 0.0],
                  [0.4, 0.7, 0.6, 0.0]], np.float64)
    T = 7.0
    want = np.zeros_like(s)
    for j in range(4):
        m = max(T * s[i][j] for i in range(3))
        l = sum(math.exp(T * s[i][j] - m) for i in range(3))
        for i in range(3):
            want[i][j] = s[i][j] * math.exp(T * s[i][j] - m) / l
    got = dual_softmax_scores(s, T)
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-14, atol=0)
    assert np.all(got[:, 3] == 0)                                     # a zero score stays zero whatever its prior
    # the softmax runs down the QUERY axis: every column of the prior sums to 1
    assert np.allclose((got / np.where(s == 0, 1, s))[:, :3].sum(0), 1.0, rtol=1e-14)
    s32 = dual_softmax_scores(s.astype(np.float32), T)
    assert s32.dtype == np.float32 and np.allclose(s32, want, rtol=1e-5)
    # the column maximum is subtracted before exp: T * s = 2000 does not overflow
    big = dual_softmax_scores(np.array([[1.0, 0.5], [0.5, 1.0]], np.float32), 2000.0)
    assert np.all(np.isfinite(big)) and big[0, 0] == 1.0 and big[1, 0] == 0.0
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            dual_softmax_scores(s, bad)


def test_temperature_zero_leaves_every_rank_unchanged():
    rng = np.random.default_rng(0)
    s = rng.standard_normal((40, 40))
    s[5] = s[6]                                                        # and a few ties
    s[:, 9] = s[:, 3]
    gt = np.arange(40)
    assert np.array_equal(dual_softmax_scores(s, 0.0), s / 40)        # the prior is 1 / Nq everywhere
    assert np.array_equal(R.stable_ranks(dual_softmax_scores(s, 0.0), gt), R.stable_ranks(s, gt))
    m = recall_for_video_text_retrieval(input_scores=s, dual_softmax=0.0)
    assert [m['DSL_' + k] for k in PLAIN] == [m[k] for k in PLAIN]


# Four texts, four videos, text i <-> video i.  Video 0 is a hub: it is the best video of texts 0, 1 and 2.
HUB = np.array([[0.9, 0.1, 0.1, 0.1],
                [0.6, 0.5, 0.1, 0.1],
                [0.6, 0.1, 0.5, 0.1],
                [0.1, 0.1, 0.1, 0.8]], np.float64)


def test_hub_video_loses_its_false_matches():
    T = 10.0
    # by hand, plain: the row maxima sit in columns 0, 0, 0, 3 -> texts 0 and 3 are right: R@1 = 50 %
    assert [int(np.argmax(r)) for r in HUB] == [0, 0, 0, 3]
    # by hand, DSL.  Column 0: T s = 9, 6, 6, 1 -> prior exp(0, -3, -3, -8) / (1 + 2 e^-3 + e^-8): the hub keeps text 0
    # (0.9 * 0.909) and is damped for texts 1 and 2 (0.6 * 0.0453 = 0.027).  Column 1: T s = 1, 5, 1, 1 -> text 1 holds
    # 1 / (1 + 3 e^-4) = 0.948 of it: 0.5 * 0.948 = 0.474 > 0.027.  Column 2 likewise for text 2.
    l0 = 1 + 2 * math.exp(-3) + math.exp(-8)
    l1 = 1 + 3 * math.exp(-4)
    sp = dual_softmax_scores(HUB, T)
    assert sp[0, 0] == pytest.approx(0.9 / l0) and sp[1, 0] == pytest.approx(0.6 * math.exp(-3) / l0)
    assert sp[1, 1] == pytest.approx(0.5 / l1) and sp[2, 2] == pytest.approx(0.5 / l1)
    assert 0.6 * math.exp(-3) / l0 < 0.5 / l1
    assert [int(np.argmax(r)) for r in sp] == [0, 1, 2, 3]
    m = recall_for_video_text_retrieval(input_scores=HUB, dual_softmax=T)
    assert list(m) == PLAIN + DSL
    assert m['Recall@1'] == 50.0 and m['DSL_Recall@1'] == 100.0
    assert m['MR'] == 1.5 and m['DSL_MR'] == 1.0                      # ranks 0 1 1 0 -> median 0.5; all 0 -> 0
    assert m['DSL_Recall@all'] == 300.0 - 1.0
    assert recall_for_video_text_retrieval(input_scores=HUB) == {k: m[k] for k in PLAIN}


def test_dsl_symbols_exported_by_both_builds():
    from clover_amd import _lib
    assert _lib.ABI_VERSION == 20
    pkg = os.path.dirname(_lib.LIB_PATH)
    i64, i32 = ctypes.c_int64, ctypes.c_int32
    for fname in ('libclover_hip_f16.so', 'libclover_hip.so'):
        so = ctypes.CDLL(os.path.join(pkg, fname))
        assert so.clv_abi_version() == 20, fname
        for name in ('clv_retrieval_col_stats_work_bytes', 'clv_retrieval_col_stats', 'clv_retrieval_rank_prior_work_bytes',
                     'clv_retrieval_rank_prior'):
            assert hasattr(so, name) and name in _lib.SIGNATURES, (fname, name)
        cs = so.clv_retrieval_col_stats_work_bytes
        cs.restype, cs.argtypes = i64, [i64, i64, i32]
        assert cs(8, 8, 6) == -2 and cs(8, 8, 4100) == -2 and cs(0, 8, 8) == -2 and cs(8, 0, 8) == -2
        # the two normalised operands + one (max, sum) pair per gallery row and query chunk (one chunk: 8 queries)
        assert cs(8, 64, 8) == (8 + 64) * 8 * 4 + 64 * 8
        # 2049 queries against 70 gallery rows: 2 gallery blocks, every one of the 33 query tiles is a chunk of its own
        assert cs(2049, 70, 64) == (2049 + 70) * 64 * 4 + 33 * 70 * 8
        rp, wb = so.clv_retrieval_rank_prior_work_bytes, so.clv_retrieval_work_bytes
        for f in (rp, wb):
            f.restype, f.argtypes = i64, [i64, i64, i32, i32]
        for shape in ((1000, 1000, 768, 0), (333, 333, 64, 10), (8, 8, 6, 0), (8, 8, 8, 17)):
            assert rp(*shape) == wb(*shape), shape
        assert wb(1000, 1000, 768, 0) == 2000 * 768 * 4                          # unchanged
        # refused before any launch (no device here): null pointers
        fn = so.clv_retrieval_col_stats
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p] * 2 + [i64, i64, i32, i64, i64, ctypes.c_float] + [ctypes.c_void_p] * 4
        assert fn(None, None, 8, 8, 8, 8, 8, 1.0, None, None, None, None) == -1
        assert fn(None, None, 8, 8, 6, 8, 8, 1.0, None, None, None, None) == -2


def test_ops_refuses_cpu_tensors():
    from clover_amd import ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_rank(torch.zeros(2, 4), torch.zeros(2, 4), dual_softmax=20.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_col_stats(torch.zeros(2, 4), torch.zeros(2, 4), 20.0)


def _embeddings(N, D, seed, caps=1):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((N, D)).astype(np.float32)
    t = (0.5 * np.repeat(v, caps, axis=0) + rng.standard_normal((N * caps, D))).astype(np.float32)
    return v, t


def test_evaluate_retrieval_adds_dsl_keys_on_host_results():
    v, t = _embeddings(30, 16, 1)
    res = dict(video_embd=v, text_embd=t)
    plain = evaluate_retrieval(res, ['recall_for_video_text_retrieval'])
    both = evaluate_retrieval(res, ['recall_for_video_text_retrieval'], dual_softmax=20.0)
    assert list(both) == PLAIN + DSL and {k: both[k] for k in PLAIN} == plain
    s = np.dot(R.restate32(t, v, 20.0)[0], np.eye(30, dtype=np.float32))
    ind = R.stable_ranks(dual_softmax_scores(s, 20.0), np.arange(30))
    assert both['DSL_Recall@1'] == float(np.sum(ind == 0)) / 30 * 100 and both['DSL_MR'] == np.median(ind) + 1
    assert both['DSL_Recall@1'] != both['Recall@1'] or both['DSL_MR'] != both['MR'] or both['DSL_Recall@5'] != both['Recall@5']
    # the many-caption metric: four keys, no Recall@all
    counts = np.array([1, 3, 2] * 10)
    vv, tt = _embeddings(30, 16, 2)
    tt = np.concatenate([np.repeat(vv[i:i + 1], c, axis=0) * 0.4 for i, c in enumerate(counts)]) + \
        np.random.default_rng(3).standard_normal((int(counts.sum()), 16)).astype(np.float32)
    var = dict(video_embd=vv, text_embd=tt.astype(np.float32), counts=counts)
    pv = evaluate_retrieval(var, ['recall_for_video_text_retrieval_varied'])
    bv = evaluate_retrieval(var, ['recall_for_video_text_retrieval_varied'], dual_softmax=20.0)
    assert list(bv) == PLAIN[:4] + DSL[:4] and {k: bv[k] for k in PLAIN[:4]} == pv
    assert bv == recall_for_video_text_retrieval_varied(vv, tt.astype(np.float32), counts, dual_softmax=20.0)
    # topk still needs device results
    with pytest.raises(ValueError, match='device results'):
        evaluate_retrieval(res, ['recall_for_video_text_retrieval'], topk=3, dual_softmax=20.0)


class _FakeModel(torch.nn.Module):
    def forward(self, return_loss=False, imgs=None, token_ids=None, **kw):
        assert not kw, kw
        return imgs.reshape(-1, imgs.shape[-1]).float(), token_ids.reshape(-1, token_ids.shape[-1]).float()


def test_eval_hook_passes_dual_softmax_on():
    from clover_amd.runner import EvalHook
    v, t = _embeddings(12, 8, 4)
    V, T = torch.from_numpy(v), torch.from_numpy(t)
    loader = [dict(imgs=V[i:i + 4, None, :], token_ids=T[i:i + 4], index=torch.arange(i, i + 4)) for i in (0, 4, 8)]
    plain = EvalHook(loader, save_best=None)
    assert plain.dual_softmax is None
    hook = EvalHook(loader, dual_softmax=20, save_best='DSL_Recall@1')
    assert hook.dual_softmax == 20.0 and hook.rule == 'greater' and hook.key_indicator == 'DSL_Recall@1'
    m0, m1 = plain._test(_FakeModel()), hook._test(_FakeModel())
    assert list(m0) == PLAIN and list(m1) == PLAIN + DSL and {k: m1[k] for k in PLAIN} == m0
    assert m1 == evaluate_retrieval(dict(video_embd=v, text_embd=t), ['recall_for_video_text_retrieval'], dual_softmax=20.0)
    with pytest.raises(ValueError, match='multiple choice'):
        EvalHook(loader, metrics=['video_qa_mc'], test_fn='recall_for_video_text_retrieval', dual_softmax=20.0)
    with pytest.raises(ValueError, match='multiple choice'):
        EvalHook(loader, test_fn='use_itm_head_fn', dual_softmax=20.0)
    with pytest.raises(ValueError, match='callable'):
        EvalHook(loader, test_fn=lambda m, l: {}, dual_softmax=20.0)


def test_the_two_refusals_name_their_reason():
    v, t = _embeddings(6, 8, 5, caps=2)
    with pytest.raises(ValueError, match='not defined for multiple choice'):
        mc_acc_on_device(v, t, np.zeros(6, np.int64), dual_softmax=20.0)
    with pytest.raises(ValueError, match='not defined for multiple choice'):
        evaluate_retrieval(dict(video_embd=v, text_embd=t, label=np.zeros(6)), ['video_qa_mc'], dual_softmax=20.0)
    with pytest.raises(ValueError, match='V2T_.*clv_retrieval_group_best'):
        recall_varied_on_device(v, t, np.full(6, 2), v2t=True, dual_softmax=20.0)
    with pytest.raises(ValueError, match='V2T_.*clv_retrieval_group_best'):
        evaluate_retrieval(dict(video_embd=v, text_embd=t, counts=np.full(6, 2)),
                           ['recall_for_video_text_retrieval_varied'], v2t=True, dual_softmax=20.0)


def _tool(name):
    spec = importlib.util.spec_from_file_location(f'clv_tools_dsl_{name}', os.path.join(ROOT, 'tools', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_config_and_cli_flag(monkeypatch):
    from clover_amd.runner import Config, EvalHook
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'finetune_retrieval_dsl_synthetic.py'))
    base = Config.fromfile(os.path.join(ROOT, 'configs', 'finetune_retrieval_synthetic.py'))
    ev = dict(cfg.evaluation)
    assert ev['dual_softmax'] == 20.0 == 1 / cfg.model['loss_type']['temperature'] and ev['save_best'] == 'DSL_Recall@1'
    assert 'dual_softmax' not in dict(base.evaluation)
    assert cfg.model == base.model and cfg.data == base.data
    hook = EvalHook([], **ev)                                         # what tools/train.py --validate builds
    assert hook.dual_softmax == 20.0 and hook.rule == 'greater'
    test = _tool('test')
    monkeypatch.setattr(sys, 'argv', ['test.py', 'cfg.py', 'ckpt.pth'])
    assert test.parse_args().dual_softmax is None
    monkeypatch.setattr(sys, 'argv', ['test.py', 'cfg.py', 'ckpt.pth', '--dual-softmax', '100', '--topk', '5', '--out', 'o'])
    a = test.parse_args()
    assert (a.dual_softmax, a.topk, a.out) == (100.0, 5, 'o')
    assert test.select_test(cfg, None) == ('retrieval', ['recall_for_video_text_retrieval'])


@pytest.mark.parametrize('T', R.TEMPERATURES)
@pytest.mark.parametrize('case', R.WINDOW_CASES + [R.WIDE_CASE], ids=lambda c: 'x'.join(map(str, c[:3])))
def test_numpy_fp32_restatement_stays_inside_the_windows(case, T):
    """What the GPU test asks of the kernels, asked of numpy in fp32 here: s' within the per-element bound, the rank
    inside [lo, hi], and the share of windows that hold more than one value under the cap."""
    c = R.window_case(case, T)
    Nq = len(c['q'])
    _, sp32 = R.restate32(c['q'], c['gal'], T)
    err = np.abs(sp32.astype(np.float64) - c['sp64'])
    rank = R.stable_ranks(sp32, c['gt'])
    print(f'{case} T={T:g} eps_s={c["eps_s"]:.3e} eps_r={R.eps_r(Nq, c["eps_s"], T):.3e} '
          f'max err/bound={float((err / c["e"]).max()):.3f} wide={100 * c["wide"]:.2f}% '
          f'outside={int(((rank < c["lo"]) | (rank > c["hi"])).sum())}')
    assert np.all(err <= c['e'])
    assert np.all((rank >= c['lo']) & (rank <= c['hi']))
    assert c['wide'] <= R.WIDE_CAP, c['wide']


def test_error_budget_terms():
    """The derived constants of tests/RETRIEVAL_DSL_ERROR_BUDGET.md, so that a change of them shows up here."""
    assert R.eps_s(64) == 2 * 68 * 2.0 ** -24
    assert R.rescales(2049) == 33 + 6 and R.rescales(64) == 1 + 6
    es = R.eps_s(96)
    assert R.eps_x(es, 100.0) == 200 * es + 400 * 2.0 ** -24
    # eps_r: twice the exponent term (the element's own and col_sum's) dominates; everything else stays below it at T = 100
    assert 2 * R.eps_x(es, 100.0) < R.eps_r(515, es, 100.0) < 3 * R.eps_x(es, 100.0)
    assert R.eps_l(515, es, 100.0) < R.eps_r(515, es, 100.0)
