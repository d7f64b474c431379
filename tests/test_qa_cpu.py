"""CPU tests of the video-QA / fill-in-the-blank host side: registry builds of the three synthetic QA configs with the
reference's parameter names and shapes, refused configurations, accuracy metrics, the synthetic batch contract, the
tools/test.py selection of the test loop, and the library's QA entry points."""
import os
import sys

import numpy as np
import pytest
import torch

import closed_form as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ('finetune_qa_mc_synthetic.py', 'finetune_qa_oe_synthetic.py', 'finetune_fib_synthetic.py')


def _cfg(name):
    from clover_amd.runner import Config
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return Config.fromfile(os.path.join(ROOT, 'configs', name))


# the reference's QA heads (mmaction/models/heads/qa_head.py:8-85, mlm_itm_head.py:56-97) at D = 768
HEAD_SHAPES = {
    'finetune_qa_mc_synthetic.py': {'qa_head.mc_vqa_classifier.1.weight': (256, 768), 'qa_head.mc_vqa_classifier.1.bias': (256,),
                                    'qa_head.mc_vqa_classifier.2.weight': (256,), 'qa_head.mc_vqa_classifier.2.bias': (256,),
                                    'qa_head.mc_vqa_classifier.4.weight': (1, 256), 'qa_head.mc_vqa_classifier.4.bias': (1,)},
    'finetune_qa_oe_synthetic.py': {'qa_head.vqa_classifier.1.weight': (384, 768), 'qa_head.vqa_classifier.1.bias': (384,),
                                    'qa_head.vqa_classifier.2.weight': (384,), 'qa_head.vqa_classifier.2.bias': (384,),
                                    'qa_head.vqa_classifier.4.weight': (1540, 384), 'qa_head.vqa_classifier.4.bias': (1540,)},
    'finetune_fib_synthetic.py': {'qa_head.vqa_classifier.1.weight': (384, 768), 'qa_head.vqa_classifier.1.bias': (384,),
                                  'qa_head.vqa_classifier.2.weight': (384,), 'qa_head.vqa_classifier.2.bias': (384,),
                                  'qa_head.vqa_classifier.4.weight': (908, 384), 'qa_head.vqa_classifier.4.bias': (908,),
                                  'itm_head.itm_projector.1.weight': (768, 768), 'itm_head.itm_projector.1.bias': (768,),
                                  'itm_head.itm_projector.3.weight': (2, 768), 'itm_head.itm_projector.3.bias': (2,)},
}


@pytest.mark.parametrize('name', CONFIGS)
def test_qa_configs_build_with_reference_head_names(name):
    import clover_amd
    cfg = _cfg(name)
    torch.manual_seed(0)
    m = clover_amd.build_model(dict(cfg.model))
    sd = m.state_dict()
    heads = {k: tuple(v.shape) for k, v in sd.items() if k.startswith(('qa_head.', 'itm_head.'))}
    assert heads == HEAD_SHAPES[name]
    assert tuple(sd['multimodal_backbone.fc_in.weight'].shape) == (768, 1024)        # Swin-B, img_in_size=1024
    assert ('multimodal_backbone.all_cls_token' in sd) == (name == 'finetune_fib_synthetic.py')
    # reference init: xavier-uniform weights (|w| <= sqrt(6 / (fan_in + fan_out))), zero biases, LayerNorm (1, 0)
    for k, shp in HEAD_SHAPES[name].items():
        v = sd[k]
        if k.endswith('.2.weight'):
            assert torch.all(v == 1)
        elif k.endswith('bias'):
            assert torch.all(v == 0)
        else:
            assert float(v.abs().max()) <= (6.0 / (shp[0] + shp[1])) ** 0.5 + 1e-6
    assert cfg.optimizer['paramwise_cfg']['custom_keys'] == {'qa_head': dict(lr_mult=10)}
    assert cfg.fp16 == dict(loss_scale='dynamic')
    assert cfg.evaluation['test_fn'] == 'use_itm_head_fn'


def test_qa_lr_mult_applies_to_the_head():
    import clover_amd
    from clover_amd.engine import paramwise_options
    cfg = _cfg('finetune_qa_oe_synthetic.py')
    m = clover_amd.build_model(dict(cfg.model))
    opts = paramwise_options(m, 0.01, cfg.optimizer['paramwise_cfg'])
    assert opts['qa_head.vqa_classifier.4.weight'][1] == 10.0
    assert opts['multimodal_backbone.fc_in.weight'][1] == 1.0


def _tiny(task, **kw):
    cfg = cf.tiny_finetune_cfg()
    cfg.update(separate_test=False, ssl_head=None, loss_type=dict(type='CrossEntropyLoss'), task=task, **kw)
    return cfg


def test_headless_and_itm_branches_refuse():
    import clover_amd
    oe = dict(type='QA_OE_Head', hidden_dim=128, num_labels=37)
    itm = dict(type='ITMHead', hidden_dim=128)
    for task in ('video_qa', 'FIB'):
        with pytest.raises(NotImplementedError):                       # neither head
            clover_amd.build_model(_tiny(task, answer_cls=True))
        with pytest.raises(NotImplementedError):                       # itm_head without qa_head
            clover_amd.build_model(_tiny(task, answer_cls=True, itm_head=itm))
        with pytest.raises(NotImplementedError):                       # answer_cls + itm_head
            clover_amd.build_model(_tiny(task, answer_cls=True, itm_head=itm, qa_head=oe))
        with pytest.raises(NotImplementedError):                       # fusion-CLS row through itm_head
            clover_amd.build_model(_tiny(task, qa_head=oe))
    m = clover_amd.build_model(_tiny('FIB', answer_mask=True, itm_head=itm, qa_head=oe))
    with pytest.raises(NotImplementedError):
        m.itm_head(torch.zeros(2, 128))
    assert m.CLV_ENCODE_KEYS == ('token_ids', 'input_mask', 'label')


def test_qa_accuracy_metrics_on_closed_form_scores():
    from clover_amd.evaluation import evaluate_qa, qa_accuracy
    scores = np.array([[0.1, 0.9, 0.0], [2.0, 1.0, 0.5], [0.0, 0.1, 0.2], [1.0, 3.0, 2.0]], dtype=np.float32)
    labels = np.array([1, 0, 0, 2])
    assert qa_accuracy(scores, labels) == 0.5
    res = dict(result=scores, label=labels)
    assert evaluate_qa(res, ['video_qa_mc']) == {'acc': 0.5}
    assert evaluate_qa(res, 'video_qa_oe') == {'overall_acc': 0.5}
    assert evaluate_qa(res, ['video_qa_mc', 'video_qa_oe']) == {'acc': 0.5, 'overall_acc': 0.5}
    with pytest.raises(KeyError):
        evaluate_qa(res, ['recall_for_video_text_retrieval'])
    with pytest.raises(ValueError):
        qa_accuracy(scores, labels[:3])


@pytest.mark.parametrize('spec', [dict(num_choices=5), dict(num_labels=1540), dict(num_labels=908, fib=True)])
def test_synthetic_qa_batch_contract(spec):
    from clover_amd.utils.qa_synthetic import MASK_ID, qa_batch
    B, L = 4, 40
    b = qa_batch(B, L, 8, seed=3, size=32, **spec)
    C = spec.get('num_choices', 1) if 'num_labels' not in spec else 1
    assert b['imgs'].shape == (B, 1, 3, 8, 32, 32)
    for k in ('token_ids', 'segment_ids', 'input_mask'):
        assert b[k].shape == (B, C, L) and b[k].dtype == torch.long
    hi = spec.get('num_labels') or spec['num_choices']
    assert b['label'].shape == (B,) and int(b['label'].min()) >= 0 and int(b['label'].max()) < hi
    ids = b['token_ids']
    assert torch.all(ids[:, :, 0] == 101)
    assert torch.equal(b['input_mask'], (ids != 0).long())
    n_mask = (ids == MASK_ID).sum(-1)
    assert torch.all(n_mask == (1 if spec.get('fib') else 0))
    assert torch.equal(qa_batch(B, L, 8, seed=3, size=32, **spec)['token_ids'], ids)         # seeded


def test_tiny_qa_models_have_the_reference_state_dict():
    """state_dict names and shapes of the three variants equal the manifests make_goldens_qa.py took from the
    reference's own models (tests/golden/g_qa.npz)."""
    import json
    import clover_amd
    import qa_cases as Q
    G = np.load(os.path.join(ROOT, 'tests', 'golden', 'g_qa.npz'))
    for kind in Q.KINDS:
        ref = json.loads(str(G[f'{kind}.manifest']))
        got = {k: list(v.shape) for k, v in clover_amd.build_model(Q.tiny_qa_cfg(kind)).state_dict().items()}
        assert got == ref, (kind, set(got) ^ set(ref))


def test_tools_test_selects_the_qa_loop():
    import importlib.util
    spec = importlib.util.spec_from_file_location('clover_tools_test', os.path.join(ROOT, 'tools', 'test.py'))
    tt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tt)
    assert tt.select_test(_cfg('finetune_qa_mc_synthetic.py'), None) == ('qa', ['video_qa_mc'])
    assert tt.select_test(_cfg('finetune_fib_synthetic.py'), None) == ('qa', ['video_qa_oe'])
    assert tt.select_test(_cfg('finetune_qa_oe_synthetic.py'), ['video_qa_oe']) == ('qa', ['video_qa_oe'])
    ret = _cfg('finetune_retrieval_synthetic.py')
    assert tt.select_test(ret, None) == ('retrieval', ['recall_for_video_text_retrieval'])     # default unchanged
    assert tt.select_test(ret, ['video_qa_mc']) == ('qa', ['video_qa_mc'])
    with pytest.raises(SystemExit):
        tt.select_test(_cfg('finetune_qa_mc_synthetic.py'), ['video_qa_mc', 'recall_for_video_text_retrieval'])


def test_qa_abi_entries_are_exported_by_both_builds():
    from clover_amd import _lib
    import ctypes
    for fname in ('libclover_hip.so', 'libclover_hip_f16.so'):
        path = os.path.join(ROOT, 'clover_amd', fname)
        so = ctypes.CDLL(path)
        for sym in ('clv_qa_answer_rows', 'clv_qa_head_fwd', 'clv_qa_mc_ce_fwd', 'clv_qa_head_bwd',
                    'clv_attn_probs_mean', 'clv_qa_head_supported'):
            getattr(so, sym)
        assert so.clv_abi_version() == _lib.ABI_VERSION == 20
        f = so.clv_qa_head_supported
        f.argtypes = [ctypes.c_int32] * 3
        assert f(768, 384, 1540) == 1 and f(128, 64, 37) == 1 and f(768, 256, 1) == 1
        assert f(2048, 384, 10) == 0 and f(768, 1024, 10) == 0


def test_fib_validation_rejects_zero_and_two_masks():
    """The eager FIB check reads the per-caption [MASK] counts the row kernel writes; on the host side it refuses any
    count other than one."""
    import clover_amd
    m = clover_amd.build_model(_tiny('FIB', answer_mask=True, qa_head=dict(type='QA_OE_Head', hidden_dim=128,
                                                                           num_labels=37)))
    m._check_masks(torch.tensor([1, 1, 1], dtype=torch.int32))
    for bad in ([1, 0, 1], [1, 2, 1]):
        with pytest.raises(ValueError):
            m._check_masks(torch.tensor(bad, dtype=torch.int32))
