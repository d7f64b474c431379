"""Host side of zero-shot multiple choice and many-caption retrieval: the numpy restatements of the reference's metrics
(mmaction/core/evaluation/accuracy.py:396-427, :465-523) on cases worked out by hand, the test loops' collection, the
dispatch in evaluate_retrieval, the synthetic loaders, the config, and the two library entry points
(clv_retrieval_group_work_bytes / clv_retrieval_group_best) as far as they go without a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from clover_amd.evaluation import (acc_for_msrvtt_mc, evaluate_retrieval, multi_gpu_test_retrieval,
                                   multi_gpu_test_retrieval_varied, recall_for_video_text_retrieval_varied)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_symbols_exported_by_both_builds():
    from clover_amd import _lib
    assert _lib.ABI_VERSION == 20
    pkg = os.path.dirname(_lib.LIB_PATH)
    for fname in ('libclover_hip_f16.so', 'libclover_hip.so'):
        so = ctypes.CDLL(os.path.join(pkg, fname))
        assert so.clv_abi_version() == 20, fname
        for name in ('clv_retrieval_group_work_bytes', 'clv_retrieval_group_best'):
            assert hasattr(so, name) and name in _lib.SIGNATURES, (fname, name)
        wb = so.clv_retrieval_work_bytes
        wb.restype, wb.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
        assert wb(1000, 1000, 768, 0) == 2000 * 768 * 4                         # unchanged
        gb = so.clv_retrieval_group_work_bytes
        gb.restype, gb.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]
        assert gb(8, 8, 6) == -2 and gb(8, 8, 4100) == -2 and gb(0, 8, 8) == -2
        # the two normalised operands + one (score, index) pair per query and gallery chunk (one chunk: a 64-row gallery)
        assert gb(8, 64, 8) == (8 + 64) * 8 * 4 + 8 * 8
        assert gb(2990, 14950, 768) >= (2990 + 14950) * 768 * 4 + 2990 * 8


def test_ops_refuses_cpu_tensors():
    from clover_amd import ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_group_best(torch.zeros(2, 4), torch.zeros(6, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_group_best(torch.zeros(2, 4), torch.zeros(6, 4), lo=torch.tensor([0, 3]), hi=torch.tensor([3, 6]),
                                 want_rank=True, eps=1e-8)


# 3 videos x 2 candidates, D = 2.  Cosines: video 0 = (1, 0): (1, 1) -> 0.707, (2, 0) -> 1: candidate 1.
# video 1 = (0, 2): (0, 5) -> 1, (1, 1) -> 0.707: candidate 0.  video 2 = (3, 3): twice the same row (1, 1): a tie, and
# argmax takes the first: candidate 0.
MC_V = np.array([[1, 0], [0, 2], [3, 3]], np.float32)
MC_T = np.array([[[1, 1], [2, 0]], [[0, 5], [1, 1]], [[1, 1], [1, 1]]], np.float32)


def test_acc_for_msrvtt_mc_by_hand():
    assert acc_for_msrvtt_mc(MC_V, MC_T.reshape(6, 2), np.array([1, 0, 0])) == {'acc': 1.0}
    m = acc_for_msrvtt_mc(MC_V, MC_T.reshape(6, 2), torch.tensor([1, 0, 1]))        # the tie's second candidate loses
    assert m == {'acc': float(np.float32(2) / np.float32(3))}
    assert acc_for_msrvtt_mc(MC_V, MC_T, [0, 1, 1])['acc'] == 0.0                   # [N, C, D] is flattened
    # without sim_matrix the raw dot decides: video 1 = (0, 2) scores (0, 5) -> 10 and (1, 1) -> 2, video 0 unchanged
    assert acc_for_msrvtt_mc(MC_V, MC_T.reshape(6, 2), [1, 0, 0], use_sim=False)['acc'] == 1.0
    # a long second candidate wins the raw dot and loses the cosine
    t = MC_T.copy()
    t[0, 0] = (9, 9)
    assert acc_for_msrvtt_mc(MC_V, t, [0, 0, 0], use_sim=False)['acc'] == 1.0
    assert acc_for_msrvtt_mc(MC_V, t, [1, 0, 0], use_sim=True)['acc'] == 1.0


# 3 videos = the unit vectors of R^3, counts [1, 3, 2].  A text (a, b, c) scores the videos in the order of a, b, c.
VR_V = np.eye(3, dtype=np.float32)
VR_T = np.array([[3, 2, 1],                 # video 0: order 0 1 2 -> rank 0
                 [3, 2, 1],                 # video 1: rank 1
                 [1, 2, 3],                 # video 1: order 2 1 0 -> rank 1
                 [0, 5, 1],                 # video 1: rank 0
                 [3, 2, 1],                 # video 2: rank 2
                 [1, 1, 4]], np.float32)    # video 2: rank 0
VR_WANT = {'Recall@1': 50.0, 'Recall@5': 100.0, 'Recall@10': 100.0, 'MR': 1.5}      # ranks 0 0 0 1 1 2: median 0.5, + 1


def test_recall_varied_by_hand():
    m = recall_for_video_text_retrieval_varied(VR_V, VR_T, [['a'], ['b', 'c', 'd'], ['e', 'f']])
    assert m == VR_WANT and list(m) == ['Recall@1', 'Recall@5', 'Recall@10', 'MR']   # no Recall@all
    assert recall_for_video_text_retrieval_varied(VR_V, VR_T, np.array([1, 3, 2])) == VR_WANT
    # only the lengths count; other lengths move the ground truth: [3, 1, 2] -> ranks 0 0 2 0 2 0
    m = recall_for_video_text_retrieval_varied(VR_V, VR_T, [3, 1, 2])
    assert m['Recall@1'] == 4 / 6 * 100 and m['MR'] == 1.0


def test_evaluate_retrieval_dispatch_on_host_results():
    res = dict(video_embd=MC_V, text_embd=MC_T, label=np.array([1, 0, 1]))
    assert evaluate_retrieval(res, ['video_qa_mc']) == {'acc': float(np.float32(2) / np.float32(3))}
    assert evaluate_retrieval(dict(res, video_embd=list(MC_V), text_embd=list(MC_T)), 'video_qa_mc')['acc'] > 0.66
    var = dict(video_embd=VR_V, text_embd=VR_T, counts=np.array([1, 3, 2]))
    assert evaluate_retrieval(var, ['recall_for_video_text_retrieval_varied']) == VR_WANT
    with pytest.raises(KeyError):
        evaluate_retrieval(res, ['zeroshot_action_recognition'])
    with pytest.raises(KeyError):
        evaluate_retrieval(dict(video_embd=MC_V, text_embd=MC_T), ['video_qa_mc'])   # no label collected
    with pytest.raises(ValueError):
        evaluate_retrieval(res, ['video_qa_mc'], with_pred=True)                     # pred comes from the device path


class _FakeModel(torch.nn.Module):
    """forward_test(separate_test=True) of a retrieval model: [B * clips, D] video rows, [B * C, D] text rows (multiple
    choice comes with one clip per video: the loop tells the two cases apart by the row counts, my_eval_hook.py:58-63)."""

    def forward(self, return_loss=False, imgs=None, token_ids=None, **kw):
        assert not kw, kw                                                            # index / label never reach the model
        return imgs.reshape(-1, imgs.shape[-1]).float(), token_ids.reshape(-1, token_ids.shape[-1]).float()


def test_mc_collection_order_labels_and_repeated_tail():
    N, C, D = 5, 3, 4
    g = torch.Generator().manual_seed(3)
    V, T = torch.randn(N, D, generator=g), torch.randn(N, C, D, generator=g)
    label = torch.tensor([2, 0, 1, 1, 0])
    batches = []
    for idx in ([3, 1], [4, 0], [2, 3]):                                             # out of order; sample 3 repeated
        # the repeated sample carries another label: the FIRST occurrence must be the one that is kept
        lb = label[idx] if idx != [2, 3] else torch.tensor([1, 2])
        batches.append(dict(imgs=V[idx][:, None, :], token_ids=T[idx], index=torch.tensor(idx), label=lb))
    model = _FakeModel().train()
    res = multi_gpu_test_retrieval(model, batches, with_label=True)
    assert model.training
    assert set(res) == {'video_embd', 'text_embd', 'index', 'label'}
    assert np.array_equal(res['index'], np.arange(N)) and np.array_equal(res['label'], label.numpy())
    assert res['text_embd'].shape == (N, C, D) and np.array_equal(res['text_embd'], T.numpy())
    assert np.allclose(res['video_embd'], V.numpy(), atol=1e-6)
    assert set(multi_gpu_test_retrieval(model, batches)) == {'video_embd', 'text_embd', 'index'}     # default unchanged
    dev = multi_gpu_test_retrieval(model, batches, with_label=True, to_host=False)
    assert torch.equal(dev['label'], label) and dev['label'].dtype == torch.int64
    with pytest.raises(KeyError):
        multi_gpu_test_retrieval(model, [{k: v for k, v in batches[0].items() if k != 'label'}], with_label=True)
    assert evaluate_retrieval(res, ['video_qa_mc']) == acc_for_msrvtt_mc(V.numpy(), T.numpy(), label.numpy())


def test_varied_collection_counts_order_and_repeated_tail():
    counts, D, clips = [2, 1, 4, 3], 4, 3
    g = torch.Generator().manual_seed(5)
    V = torch.randn(len(counts), D, generator=g)
    T = [torch.randn(c, D, generator=g) for c in counts]
    d = torch.linspace(-1, 1, clips)[None, :, None]
    batches = [dict(imgs=V[i][None, None, :] + d, token_ids=T[i][None], index=torch.tensor([i])) for i in (2, 0, 3, 1, 2)]
    res = multi_gpu_test_retrieval_varied(_FakeModel(), batches)
    assert np.array_equal(res['index'], np.arange(4)) and np.array_equal(res['counts'], counts)
    assert res['text_embd'].shape == (sum(counts), D) and np.array_equal(res['text_embd'], torch.cat(T).numpy())
    assert np.allclose(res['video_embd'], V.numpy(), atol=1e-6)
    dev = multi_gpu_test_retrieval_varied(_FakeModel(), batches, to_host=False)
    assert torch.equal(dev['counts'], torch.tensor(counts)) and torch.equal(dev['text_embd'], torch.cat(T))
    m = evaluate_retrieval(res, ['recall_for_video_text_retrieval_varied'])
    assert m == recall_for_video_text_retrieval_varied(V.numpy(), torch.cat(T).numpy(), counts)
    with pytest.raises(ValueError, match='one video per batch'):
        multi_gpu_test_retrieval_varied(_FakeModel(), [dict(batches[0], index=torch.tensor([0, 1]))])


def test_synthetic_loader_candidates_and_captions():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from clover_amd.utils.synthetic_loaders import SyntheticTestLoader
    ld = SyntheticTestLoader(pairs=5, batch=2, frames=2, tokens=8, rank=0, world=1, device='cpu', candidates=5)
    assert [b['index'].tolist() for b in ld] == [[0, 1], [2, 3], [4]]
    labels = []
    for b in ld:
        B = len(b['index'])
        assert set(b) == {'imgs', 'token_ids', 'segment_ids', 'input_mask', 'label', 'index'}
        assert b['imgs'].shape[:2] == (B, 1)
        for k in ('token_ids', 'segment_ids', 'input_mask'):
            assert b[k].shape == (B, 5, 8), (k, b[k].shape)
        assert b['label'].shape == (B,) and b['label'].dtype == torch.int64
        assert bool((b['token_ids'][:, :, 0] == 101).all())                         # every candidate is a caption
        assert not torch.equal(b['token_ids'][:, 0], b['token_ids'][:, 1])
        labels += b['label'].tolist()
    assert all(0 <= x < 5 for x in labels)
    again = SyntheticTestLoader(pairs=5, batch=2, frames=2, tokens=8, rank=0, world=1, device='cpu', candidates=5)
    assert all(torch.equal(a['token_ids'], b['token_ids']) and torch.equal(a['label'], b['label'])
               for a, b in zip(ld, again))
    var = SyntheticTestLoader(pairs=5, batch=2, frames=2, tokens=8, rank=0, world=1, device='cpu', captions=[1, 3, 2])
    assert [b['index'].tolist() for b in var] == [[0], [1], [2], [3], [4]]           # unequal counts: one video per batch
    assert [tuple(b['token_ids'].shape) for b in var] == [(1, c, 8) for c in (1, 3, 2, 1, 3)]
    assert all('label' not in b for b in var)
    same = SyntheticTestLoader(pairs=5, batch=2, frames=2, tokens=8, rank=1, world=2, device='cpu', captions=2)
    assert [b['index'].tolist() for b in same] == [[1, 3]] and same.batches[0]['token_ids'].shape == (2, 2, 8)
    with pytest.raises(ValueError):
        SyntheticTestLoader(pairs=5, batch=2, frames=2, tokens=8, rank=0, world=1, device='cpu', candidates=5, captions=2)


def test_eval_hook_routes_by_metrics(monkeypatch):
    from clover_amd.runner import EvalHook
    h = EvalHook([], metrics=['video_qa_mc'], test_fn='recall_for_video_text_retrieval', save_best='acc')
    assert h.metrics == ['video_qa_mc'] and h.rule == 'greater' and h.test_fn == 'recall_for_video_text_retrieval'
    assert EvalHook([], metrics='recall_for_video_text_retrieval_varied', save_best=None).test_fn is None
    with pytest.raises(KeyError):
        EvalHook([], test_fn='zeroshot_action_recognition')
    # the loop the hook runs: labels are collected for 'video_qa_mc', the varied loop for the varied metric
    N, C, D = 4, 2, 4
    g = torch.Generator().manual_seed(9)
    V, T = torch.randn(N, D, generator=g), torch.randn(N, C, D, generator=g)
    seen = {}

    def fake_eval(res, metrics):
        seen.update(res)
        return {'acc': 0.5}
    import clover_amd.evaluation as ev
    h.dataloader = [dict(imgs=V[:, None, :], token_ids=T, index=torch.arange(N), label=torch.tensor([0, 1, 1, 0]))]
    monkeypatch.setattr(ev, 'evaluate_retrieval', fake_eval)
    assert h._test(_FakeModel()) == {'acc': 0.5}
    assert seen['label'].tolist() == [0, 1, 1, 0] and seen['text_embd'].shape == (N, C, D)


def test_mc_config_loads_and_routes():
    import importlib.util
    from clover_amd.runner import Config
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'finetune_msrvtt_mc_synthetic.py'))
    assert cfg.model['task'] == 'retrieval' and cfg.model['separate_test'] is True
    ev = dict(cfg.evaluation)
    assert ev['metrics'] == ['video_qa_mc'] and ev['test_fn'] == 'recall_for_video_text_retrieval'
    assert ev['save_best'] == 'acc' and cfg.data['synthetic_test']['candidates'] == 5
    from clover_amd.runner import EvalHook
    assert EvalHook([], **ev).rule == 'greater'                                     # what tools/train.py --validate builds
    spec = importlib.util.spec_from_file_location('clv_tools_test_mc', os.path.join(ROOT, 'tools', 'test.py'))
    tt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tt)
    assert tt.select_test(cfg, None) == ('retrieval', ['video_qa_mc'])
    assert tt.select_test(cfg, ['video_qa_mc']) == ('retrieval', ['video_qa_mc'])
    ret = Config.fromfile(os.path.join(ROOT, 'configs', 'finetune_retrieval_synthetic.py'))
    assert tt.select_test(ret, ['recall_for_video_text_retrieval_varied']) == ('retrieval',
                                                                               ['recall_for_video_text_retrieval_varied'])
