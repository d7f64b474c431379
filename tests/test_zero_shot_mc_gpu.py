"""Zero-shot multiple choice end to end on the tiny closed-form CloverFinetune: synthetic test set -> test loop with
labels -> evaluate_retrieval(['video_qa_mc']) on the device, against the host metric on the same embeddings; and one
EvalHook epoch that records `acc` and keeps the best checkpoint.  `-m gpu` only."""
import os

import numpy as np
import pytest
import torch

from test_engine_gpu import batch, make_finetune_model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
C = 5


def mc_loader():
    """6 videos with 5 candidate captions each, in batches of 2, at the tiny model's clip size and vocabulary."""
    from clover_amd.utils.synthetic_loaders import SyntheticTestLoader
    return SyntheticTestLoader(pairs=6, batch=2, frames=4, tokens=16, rank=0, world=1, device=DEV, candidates=C,
                               size=112, vocab=1024)


def test_chain_against_host_metric():
    from clover_amd.evaluation import acc_for_msrvtt_mc, evaluate_retrieval, multi_gpu_test_retrieval
    m, loader = make_finetune_model(), mc_loader()
    b0 = loader.batches[0]
    assert b0['token_ids'].shape == (2, C, 16) and int(b0['token_ids'].max()) < 1024
    v, t = m(return_loss=False, **{k: b0[k] for k in ('imgs', 'token_ids', 'segment_ids', 'input_mask')})
    assert v.shape == (2, 128) and t.shape == (2 * C, 128)        # [B, D] / [B*C, D], multimodal_transformer_finetune.py:138-154
    res = multi_gpu_test_retrieval(m, loader, with_label=True, to_host=False)
    assert res['video_embd'].shape == (6, 128) and res['text_embd'].shape == (6, C, 128) and res['label'].shape == (6,)
    assert res['video_embd'].is_cuda and res['index'].tolist() == list(range(6))
    got = evaluate_retrieval(res, ['video_qa_mc'], with_pred=True)
    assert evaluate_retrieval(res, ['video_qa_mc']) == {'acc': got['acc']}
    ve, te, label = (res[k].cpu().numpy() for k in ('video_embd', 'text_embd', 'label'))
    host = acc_for_msrvtt_mc(ve, te.reshape(-1, 128), label, use_sim=True)
    # fp64 cosines of the same embeddings: where the best candidate leads by more than 2 eps_s the device must pick it
    D = 128
    eps_s = 2 * (D + 4) * 2.0 ** -24
    v64, t64 = ve.astype(np.float64), te.astype(np.float64)
    s = np.einsum('nd,ncd->nc', v64 / np.linalg.norm(v64, axis=1, keepdims=True),
                  t64 / np.linalg.norm(t64, axis=2, keepdims=True))
    top2 = -np.sort(-s, axis=1)[:, :2]
    clear = top2[:, 0] - top2[:, 1] > 2 * eps_s
    print('fp64 top-2 gaps', top2[:, 0] - top2[:, 1], 'device pred', got['pred'], 'label', label, 'acc', got['acc'], host)
    assert clear.sum() >= 5
    assert np.array_equal(got['pred'][clear], np.argmax(s, axis=1)[clear])
    if clear.all():
        assert got['acc'] == host['acc']
    assert got['acc'] == float((got['pred'] == label).astype(np.float32).mean())


def test_eval_hook_epoch_records_acc_and_keeps_best(tmp_path):
    from clover_amd.engine import CloverEngine
    from clover_amd.runner import CloverRunner, EvalHook
    b = batch(2, 'mchook')
    m = make_finetune_model().train()
    eng = CloverEngine(m, b, lr=1e-3, weight_decay=0.0, grad_clip=15.0, max_iters=10 ** 9)
    wd = tmp_path / 'mc'
    runner = CloverRunner(eng, model=m, work_dir=str(wd), max_epochs=1)
    hook = EvalHook(mc_loader(), metrics=['video_qa_mc'], test_fn='recall_for_video_text_retrieval', save_best='acc')
    runner.register_hook(hook)
    runner.run([[b]], [('train', 1)], 1)                           # _guard raises if the evaluation disturbed the training
    torch.cuda.synchronize()
    assert m.training
    assert len(hook.records) == 1 and set(hook.records[0]) == {'epoch', 'mode', 'acc'}
    acc = hook.records[0]['acc']
    assert acc in [float(np.float32(k) / np.float32(6)) for k in range(7)]
    assert os.listdir(str(wd)) == ['mc_best_acc_epoch_1.pth']
    assert runner.meta['hook_msgs']['best_score'] == acc
    ck = torch.load(os.path.join(str(wd), 'mc_best_acc_epoch_1.pth'), map_location='cpu')
    assert ck['meta']['hook_msgs']['best_score'] == acc
