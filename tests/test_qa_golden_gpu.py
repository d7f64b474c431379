"""The video-QA / fill-in-the-blank path against the REAL reference: tests/golden/g_qa.npz, written by
tests/golden/make_goldens_qa.py from CloverFinetune(task='video_qa' / 'FIB') of the reference on the closed-form weights
and batches of tests/golden/qa_cases.py (eval mode: dropout off).  `-m gpu` only."""
import json
import os

import numpy as np
import pytest
import torch

import closed_form as cf
import qa_cases as Q

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g_qa.npz'))
MAXSUB = 1024              # make_goldens_qa.pack


def sub(t):
    a = t.detach().float().cpu().double().numpy().reshape(-1)
    return a[::max(1, a.size // MAXSUB)][:MAXSUB]


def rel(a, ref, floor=1e-5):
    """max|a - ref| / max|ref|; the floor stands in for gradients that are zero in exact arithmetic (the multiple-choice
    score bias: softmax - onehot sums to zero over each sample's candidates)."""
    return float(np.abs(a - ref).max()) / max(float(np.abs(ref).max()), floor)


def model(kind):
    import clover_amd
    m = clover_amd.build_model(Q.tiny_qa_cfg(kind))
    manifest = json.loads(str(G[f'{kind}.manifest']))
    missing, unexpected = m.load_state_dict(cf.cf_state(manifest), strict=False)
    assert not unexpected and all('relative_position_index' in k for k in missing), (missing, unexpected)
    return m.to(DEV).eval()


@pytest.mark.parametrize('B', [2, 4])
@pytest.mark.parametrize('kind', Q.KINDS)
def test_qa_step_and_forward_test_match_the_reference(kind, B):
    m = model(kind)
    batch = {k: v.to(DEV) for k, v in Q.qa_batch(kind, B, f'qa.{kind}.B{B}').items()}
    out = m.train_step(batch)
    out['loss'].backward()
    pre = f'{kind}.B{B}.'
    assert abs(float(out['log_vars']['qa_loss']) - float(G[pre + 'qa_loss'])) <= 5e-3
    named = dict(m.named_parameters())
    keys = [k[len(pre + 'grad.'):-len('.sub')] for k in G.files if k.startswith(pre + 'grad.') and k.endswith('.sub')]
    assert len(keys) >= 10
    for k in keys:
        assert named[k].grad is not None, k
        r = rel(sub(named[k].grad), G[pre + f'grad.{k}.sub'])
        assert r <= 5e-2, (k, r)
    assert sum(p.grad is None for p in named.values()) == int(G[pre + 'n_unused'])
    with torch.no_grad():
        res = m(return_loss=False, imgs=batch['imgs'], token_ids=batch['token_ids'],
                segment_ids=batch['segment_ids'], input_mask=batch['input_mask'])
    ref = G[pre + 'result']
    got = res['result'].cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32
    assert rel(got, ref) <= 2e-2
    assert float(np.abs(sub(res['attention']) - G[pre + 'attention.sub']).max()) <= 1e-3


@pytest.mark.parametrize('M,K', Q.HEAD_CASES)
def test_heads_alone_at_bert_base_width(M, K):
    import clover_amd
    from clover_amd.builder import build_head
    head = build_head(dict(type='QA_MC_head', hidden_dim=768) if K == 1
                      else dict(type='QA_OE_Head', hidden_dim=768, num_labels=K))
    head.load_state_dict(cf.cf_state({k: list(v.shape) for k, v in head.state_dict().items()}))
    head = head.to(DEV).eval()
    tag = f'head.M{M}.K{K}'
    x = cf.cf_float(tag + '.x', (M, 768), 1.0).to(DEV).requires_grad_()
    y = head(x)
    assert rel(sub(y), G[tag + '.y.sub']) <= 2e-2          # (the kernel reads the rows in the 16-bit element type)
    y.backward(cf.cf_float(tag + '.dy', tuple(y.shape), 1.0).to(DEV))
    assert rel(sub(x.grad), G[tag + '.dx.sub']) <= 5e-2
    for n, p in head.named_parameters():
        assert rel(sub(p.grad), G[f'{tag}.grad.{n}.sub']) <= 5e-2, n
    del clover_amd
